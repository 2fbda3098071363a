#!/usr/bin/env python3
"""The acoustic tokenizer measured: 32 clips of 6 s (563 mel frames each, log-mel-like values) through
the full-size encoder (channels 100, hidden 512, 3 ResBlocks, codebook 512 x 8192) at seeded weights, in ONE process with the
arms alternating round by round:
  (a) the functional torch form on the device, clip by clip (indextts/vqvae/dvae.py: encoder_forward, nearest_code -- fp32
      conv1d and matmul of the framework's libraries);
  (b) CodecEngine.encode of the ragged batch: twelve ittc_conv and one ittc_nearest_code.
Each arm between two device events, median of 7 after two warm-up rounds; for (b) also every launch between two device events
behind a queued spin kernel (the host's enqueueing is not in the span).  No ratio is fixed in advance: the output is the record.
The two arms' codes are compared and the number of differing frames is printed (seeded weights leave frames undecided: fp32 in
two summation orders).  Writes profiles/codec.txt.
usage: bench_codec.py [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from indextts import _native_codec as natc  # noqa: E402
from indextts.vqvae.dvae import CodecEngine, code_count, encoder_forward, nearest_code  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_codec.py measures on the GPU: none is visible")
DEV, REPS, WARM, SPIN_CYCLES = torch.device("cuda:0"), 7, 2, 2_000_000
CLIPS, SECONDS = 32, 6.0
T = int(SECONDS * 24000) // 256 + 1
CH, HID, CD, NT, NRES = 100, 512, 512, 8192, 3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return f"{statistics.median(v):.1f}  [{min(v):.1f} .. {max(v):.1f}]"


g = torch.Generator().manual_seed(26)


def conv_w(co, ci, k):
    bound = (ci * k) ** -0.5
    return (torch.rand(co, ci, k, generator=g) * 2 - 1) * bound, (torch.rand(co, generator=g) * 2 - 1) * bound


sd = {}
for key, (co, ci, k) in {"encoder.0.0": (HID, CH, 3), "encoder.1.0": (2 * HID, HID, 3), f"encoder.{2 + NRES}": (CD, 2 * HID, 1)}.items():
    sd[key + ".weight"], sd[key + ".bias"] = conv_w(co, ci, k)
for i in range(NRES):
    for n, k in ((0, 3), (2, 3), (4, 1)):
        sd[f"encoder.{2 + i}.net.{n}.weight"], sd[f"encoder.{2 + i}.net.{n}.bias"] = conv_w(2 * HID, 2 * HID, k)
sd["codebook.embed"] = torch.randn(CD, NT, generator=g)
sd_dev = {k: v.to(DEV) for k, v in sd.items()}
engine = CodecEngine(sd, DEV)
mels = [(torch.rand(CH, T, generator=g) * 8.0 - 6.0).to(DEV) for _ in range(CLIPS)]


def arm_a():
    return [nearest_code(encoder_forward(sd_dev, m), sd_dev["codebook.embed"]) for m in mels]


def arm_b():
    return engine.encode(mels)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


ta, tb = [], []
for rep in range(WARM + REPS):
    a, ca = timed(arm_a)
    b, cb = timed(arm_b)
    if rep >= WARM:
        ta.append(a), tb.append(b)
frames = sum(int(c.numel()) for c in cb)
differ = sum(int((x != y).sum()) for x, y in zip(ca, cb))
assert all(int(c.numel()) == code_count(T) for c in cb)
audio = CLIPS * SECONDS
say(f"{CLIPS} clips of {SECONDS:g} s ({T} mel frames, {code_count(T)} codes each; {frames} codes); full-size encoder, seeded weights, fp32; us, "
    f"median of {REPS} [min .. max] between device events, the arms alternating in one process")
say(f"(a) torch functional form, clip by clip: {med(ta)}  = {audio / (statistics.median(ta) * 1e-6):.0f} audio-s/s")
say(f"(b) CodecEngine.encode, ragged batch:    {med(tb)}  = {audio / (statistics.median(tb) * 1e-6):.0f} audio-s/s")
say(f"(b) / (a) = {statistics.median(tb) / statistics.median(ta):.3f}; {differ} of {frames} codes differ between the arms")

# every launch of (b) between device events behind a queued spin kernel
spans = []
real = {k: getattr(natc, k) for k in ("conv", "nearest_code")}


def wrap(name):
    def wrapped(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(SPIN_CYCLES)
        e0.record()
        r = real[name](*a, **kw)
        e1.record()
        spans.append((name, e0, e1))
        return r
    return wrapped


for k in real:
    setattr(natc, k, wrap(k))
per = None
try:
    for rep in range(WARM + 5):
        spans.clear()
        engine.encode(mels)
        torch.cuda.synchronize()
        row = [e0.elapsed_time(e1) * 1e3 for _, e0, e1 in spans]
        if rep >= WARM:
            per = [row] if per is None else per + [row]
finally:
    for k in real:
        setattr(natc, k, real[k])
names = [L["key"] for L in engine.layers] + ["nearest_code"]
lens = [T]
for L in engine.layers:
    lens.append(natc.out_rows(lens[-1], L["stride"]))
say("per launch of (b), median of 5:")
for i, name in enumerate(names):
    v = [r[i] for r in per]
    if i < len(engine.layers):
        L = engine.layers[i]
        fl = 2.0 * CLIPS * lens[i + 1] * L["Cout"] * L["Cin"] * L["taps"]
        what = f"{L['Cin'] * L['taps']} -> {L['Cout']}, stride {L['stride']}, {CLIPS * lens[i + 1]} rows"
    else:
        fl = 2.0 * frames * CD * NT
        what = f"{frames} rows x {NT} codes x {CD}"
    say(f"  {name:18s} {what:42s} {med(v)}  {fl / (statistics.median(v) * 1e-6) / 1e12:.1f} TFLOP/s")
say(f"  sum of the launches: {sum(statistics.median([r[i] for r in per]) for i in range(len(names))):.1f}")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
