#!/usr/bin/env python3
"""The prompt audio front-end measured: decoded waveform in host memory -> log-mel on the device.
Timed region: a host clock from the decoded planar waveform(s) in host memory to the mel(s) on the device, synchronised; median
of 9 after two warm-up rounds; the arms alternate inside one process.
  (a) today's path: the torch ops on the host (channel mean, feature_extractors.resample, MelSpectrogramFeatures), then the upload
  (b) the same torch ops on device tensors (the upload first), if the installed torch can: "unavailable" if torch.stft raises
  (c) PromptAudioEngine.mel: one upload, one itta_resample launch per rate, one itta_logmel launch
Inputs: tests/golden/sample_prompt.wav (44.1 kHz stereo, 5.4 s), and a batch of eight seeded prompts of 3-12 s (44.1 kHz stereo and
mono, 48 kHz, 16 kHz, 24 kHz).  (a) and (b) take a batch one prompt after the other, as IndexTTS does today; (c) in one pass.
Beside them the two kernels' own times: each launch alone between two device events (no graph), median of 9.  A spin kernel of
about a millisecond is queued ahead of the first event, so the host has enqueued event, launch and event before the device
reaches them: the span holds the kernel, not the host's launch latency.
No ratio is fixed in advance: the output is the record.  Writes the section "timing" of profiles/prompt_frontend.txt and keeps
what the file holds from its line "accuracy" on (put there by hand from tests/test_prompt_frontend_gpu.py -s).
usage: bench_prompt_frontend.py [--out FILE]"""
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

from indextts.utils.audio import read_audio  # noqa: E402
from indextts.utils.audio_engine import PromptAudioEngine  # noqa: E402
from indextts.utils.feature_extractors import MelSpectrogramFeatures, resample  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_frontend.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_prompt_frontend.py measures on the GPU: none is visible")
DEV, REPS, WARM = torch.device("cuda:0"), 9, 2
SPIN_CYCLES = 2_000_000
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


audio, sr0 = read_audio(os.path.join(ROOT, "tests", "golden", "sample_prompt.wav"))
sample = (torch.from_numpy(audio.T if audio.ndim > 1 else audio.reshape(1, -1)).float().contiguous(), sr0)
rng = np.random.default_rng(11)
SPEC = [(2, 3.0, 44100), (1, 4.5, 44100), (2, 6.0, 48000), (1, 7.0, 16000), (1, 8.5, 24000), (2, 10.0, 44100), (1, 11.0, 48000), (2, 12.0, 44100)]
batch = [(torch.from_numpy(rng.uniform(-0.5, 0.5, size=(c, int(sec * sr))).astype(np.float32)), sr) for c, sec, sr in SPEC]
extractor = MelSpectrogramFeatures()
engine = PromptAudioEngine(DEV)


def arm_host(items):
    return [extractor(resample(torch.mean(x, dim=0, keepdim=True), sr, 24000)).to(DEV) for x, sr in items]


def arm_device(items):
    return [extractor(resample(torch.mean(x.to(DEV), dim=0, keepdim=True), sr, 24000)) for x, sr in items]


def arm_hip(items):
    return engine.mel([x for x, _ in items], [sr for _, sr in items])


def timed(fn, items):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(items)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


say("timing  (host clock, decoded waveform in host memory -> mel on the device, synchronised; ms, median of 9 [min .. max])")
for name, items in (("sample_prompt.wav, one prompt", [sample]), ("eight prompts of 3-12 s", batch)):
    arms = [("(a) torch ops on the host + upload", arm_host), ("(b) torch ops on the device", arm_device), ("(c) HIP engine", arm_hip)]
    try:
        arm_device(items[:1])
    except Exception as e:  # noqa: BLE001
        arms[1] = (arms[1][0], None)
        why = f"unavailable ({type(e).__name__}: {str(e).splitlines()[0][:80]})"
    times, outs = {n: [] for n, _ in arms}, {}
    for rep in range(WARM + REPS):
        for n, fn in arms:                       # alternating: every arm once per round
            if fn is None:
                continue
            ms, out = timed(fn, items)
            outs[n] = out
            if rep >= WARM:
                times[n].append(ms)
    frames = sum(int(m.shape[-1]) for m in outs[arms[2][0]])
    say(f"  {name}: {frames} frames")
    for n, fn in arms:
        if fn is None:
            say(f"    {n}: {why}")
            continue
        t = times[n]
        say(f"    {n}: {statistics.median(t):.3f}  [{min(t):.3f} .. {max(t):.3f}]")
    ref = outs[arms[0][0]]
    for n, fn in arms[1:]:
        if fn is not None:
            d = max(float((a.exp() - b.exp()).abs().div(a.exp() + 1e-7).max()) for a, b in zip(outs[n], ref))
            say(f"    {n} against (a), max |d| / (mel + 1e-7) in the linear domain: {d:.3e}")

say("kernels alone  (each launch between two device events behind a queued spin kernel, no graph; us, median of 9 [min .. max])")
for name, items in (("sample_prompt.wav, one prompt", [sample]), ("eight prompts of 3-12 s", batch)):
    from indextts import _native_audio as nata
    spans = {}
    real_r, real_m = nata.resample, nata.logmel

    def wrap(kind, fn):
        def inner(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN_CYCLES)       # keeps the stream busy while the host enqueues what follows
            e0.record()
            r = fn(*a)
            e1.record()
            spans.setdefault(kind, []).append((e0, e1))
            return r
        return inner

    per = {"itta_resample (all rates)": [], "itta_logmel": []}
    nata.resample, nata.logmel = wrap("r", real_r), wrap("m", real_m)
    try:
        for rep in range(WARM + REPS):
            spans.clear()
            arm_hip(items)
            torch.cuda.synchronize()
            if rep >= WARM:
                per["itta_resample (all rates)"].append(sum(a.elapsed_time(b) for a, b in spans["r"]) * 1e3)
                per["itta_logmel"].append(sum(a.elapsed_time(b) for a, b in spans["m"]) * 1e3)
    finally:
        nata.resample, nata.logmel = real_r, real_m
    say(f"  {name}:")
    for k, t in per.items():
        say(f"    {k}: {statistics.median(t):.1f}  [{min(t):.1f} .. {max(t):.1f}]")

keep = []
if os.path.exists(args.out):
    old = open(args.out).read().splitlines()
    for i, ln in enumerate(old):
        if ln.startswith("accuracy"):
            keep = old[i:]
            break
with open(args.out, "w") as f:
    f.write("\n".join(lines + keep) + "\n")
