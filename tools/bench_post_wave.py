#!/usr/bin/env python3
"""Waveform finishing measured: 32 utterances of 6 s (fp32 at 24 kHz on the device; speech-like bursts
at different levels between silences, tests/post_wave_refs.bursts) -> trimmed, pauses capped at 100 ms, -20 dBFS, fp32 on the
device.  Timed region: a host clock from the waveforms on the device to the finished waveforms on the device, synchronised;
median of 9 after two warm-up rounds; the arms alternate inside one process.
  (a) today's only route: device -> host of the fp32 samples, numpy framing, the plan, numpy splicing, host -> device
  (b) the same steps as torch ops on the device tensors (framing by reshape, the statistics' copy, the plan, slicing and cat)
  (c) PostWaveEngine.process: ittp_frame_stats, the statistics' copy, the plan, ittp_splice
All three run the SAME plan function on their own statistics.  Beside them: each kernel alone between two device events behind a
queued spin kernel (bench_pcm_out.py's method), with the bytes it moves and the time those bytes take at the 8 TB/s HBM peak
DESIGN.md section 5 uses, and the size of the statistics' copy.
No ratio is fixed in advance: the output is the record.  Writes profiles/post_wave.txt.
usage: bench_post_wave.py [--out FILE]"""
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

import post_wave_refs as R  # noqa: E402
from indextts import _native_post as natp  # noqa: E402
from indextts.utils.post_wave import FRAME, PostProcess, PostWaveEngine, plan, ramp_table  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_wave.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_post_wave.py measures on the GPU: none is visible")
DEV, REPS, WARM, SPIN_CYCLES, HBM = torch.device("cuda:0"), 9, 2, 2_000_000, 8.0e12
ROWS, SECONDS = 32, 6
PP = PostProcess(trim_db=-45.0, max_pause_ms=100.0, target_rms_db=-20.0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


# 600 frames a row: 0.4 s of silence, speech, a pause of 0.3 .. 0.9 s, speech, silence; every row at a level of its own
waves = []
for r in range(ROWS):
    gap = 30 + 2 * r
    first = (600 - 40 - gap - 60) // 2
    layout = [("q", 40), ("s", first), ("q", gap), ("s", 600 - 40 - gap - 60 - first), ("q", 60)]
    waves.append(torch.from_numpy(R.bursts(layout, seed=r, floor_db=-70.0, burst_db=-30.0 + 0.6 * r)).to(DEV))
assert all(int(w.numel()) == SECONDS * 24000 for w in waves)
engine = PostWaveEngine(DEV)
RAMP_H = ramp_table().numpy()
RAMP_D = ramp_table().to(DEV)


def splice_with(x, pl, ramp, cat):
    parts = []
    for src, _, n, fi, fo in pl.pieces:
        seg = x[src:src + n] * float(pl.gain)                    # (a copy, fp32 in both worlds)
        if fi:
            seg[:fi] *= ramp
        if fo:
            seg[n - fo:] *= ramp.flip(0) if torch.is_tensor(ramp) else ramp[::-1]
        parts.append(seg)
    return cat(parts)


def arm_host(_):
    out, moved = [], 0
    for w in waves:
        h = w.cpu().numpy()
        moved += h.size * 4
        pad = np.concatenate([h, np.zeros(-h.size % FRAME, dtype=np.float32)]).reshape(-1, FRAME)
        st = np.stack([(pad * pad).sum(1), np.abs(pad).max(1)], 1)
        y = splice_with(h, plan(st, h.size, PP), RAMP_H, np.concatenate)
        moved += y.size * 4
        out.append(torch.from_numpy(y).to(DEV))
    return out, moved


def arm_device(_):
    out, moved = [], 0
    for w in waves:
        pad = torch.nn.functional.pad(w, (0, -int(w.numel()) % FRAME)).view(-1, FRAME)
        st = torch.stack([(pad * pad).sum(1), pad.abs().amax(1)], 1).cpu().numpy()
        moved += st.size * 4
        out.append(splice_with(w, plan(st, int(w.numel()), PP), RAMP_D, torch.cat))
    return out, moved


def arm_hip(_):
    out = engine.process(waves, PP)
    return out, sum(-(-int(w.numel()) // FRAME) for w in waves) * 8


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


say(f"timing  ({ROWS} rows of {SECONDS} s; {PP}; host clock, fp32 on the device -> finished fp32 on the device, synchronised; "
    f"ms, median of {REPS} [min .. max])")
arms = [("(a) device -> host, numpy framing + plan + splice, host -> device", arm_host),
        ("(b) the torch ops on the device, the statistics to the host for the plan", arm_device),
        ("(c) HIP engine: ittp_frame_stats, the statistics to the host for the plan, ittp_splice", arm_hip)]
times, outs = {n: [] for n, _ in arms}, {}
for rep in range(WARM + REPS):
    for n, fn in arms:                       # alternating: every arm once per round
        ms, out = timed(fn)
        outs[n] = out
        if rep >= WARM:
            times[n].append(ms)
med = {}
for n, _ in arms:
    t = times[n]
    med[n] = statistics.median(t)
    say(f"    {n}: {med[n]:.3f}  [{min(t):.3f} .. {max(t):.3f}]   {outs[n][1]} bytes between device and host")
c = arms[2][0]
say(f"    (c) against (a): {med[arms[0][0]] / med[c]:.2f} x; against (b): {med[arms[1][0]] / med[c]:.2f} x")
kept = sum(int(o.numel()) for o in outs[c][0])
say(f"    samples kept: {kept} of {ROWS * SECONDS * 24000}")
for n, _ in arms[:2]:
    same = all(a.shape == b.shape for a, b in zip(outs[n][0], outs[c][0]))
    worst = max(float(((a - b).abs() / b.abs().clamp(min=1e-3)).max()) for a, b in zip(outs[n][0], outs[c][0])) if same else float("nan")
    say(f"    {n[:3]} against (c): the same lengths: {same}; largest relative difference of a sample {worst:.3g} "
        f"(sums in another order move the gain)")

say(f"kernels alone  (the launch between two device events behind a queued spin kernel, no graph; us, median of {REPS} [min .. max]; "
    f"bytes at the {HBM / 1e12:g} TB/s HBM peak)")
n_in = ROWS * SECONDS * 24000
for name, moved in (("frame_stats", n_in * 4 + (n_in // FRAME) * 8), ("splice", kept * 8)):
    real, spans, per = getattr(natp, name), [], []

    def wrapped(*a, _real=real):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(SPIN_CYCLES)       # keeps the stream busy while the host enqueues what follows
        e0.record()
        r = _real(*a)
        e1.record()
        spans.append((e0, e1))
        return r

    setattr(natp, name, wrapped)
    try:
        for rep in range(WARM + REPS):
            spans.clear()
            engine.process(waves, PP)
            torch.cuda.synchronize()
            if rep >= WARM:
                per.append(sum(a.elapsed_time(b) for a, b in spans) * 1e3)
    finally:
        setattr(natp, name, real)
    t = statistics.median(per)
    say(f"  ittp_{name}: {t:.1f}  [{min(per):.1f} .. {max(per):.1f}]   {moved} bytes (frame_stats: the samples read, the statistics written; splice: the kept samples read and written): "
        f"{moved / HBM * 1e6:.1f} us at the peak, {moved / (t * 1e-6) / 1e12:.2f} TB/s achieved")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
