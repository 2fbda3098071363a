#!/usr/bin/env python3
"""The speaking rate measured: 1 and 32 utterances of 10 s (fp32 at 24 kHz on the device, speech-like:
tests/tempo_refs.speechlike) at the speeds 0.8 and 1.25 -> the two launches of TempoEngine.process, ittm_search and
ittm_overlap_add, each between two device events behind a queued spin kernel (the host's enqueueing is not in the span);
median of 9 after two warm-up rounds.  Beside them, in the same run: BigVGAN.forward (fp16, the synthetic weights of
tests/weights.py) over the latents of the same rows -- 938 frames a row -- between device events, median of 5 after one warm-up.
ittm_search walks a row's chain in ONE workgroup: its time is that of the longest row, whatever the batch, up to one row per CU.
No threshold is fixed in advance: the output is the record.  Writes profiles/tempo.txt.
usage: bench_tempo.py [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import tempo_refs as R  # noqa: E402
import weights  # noqa: E402
from indextts import _native_tempo as natm  # noqa: E402
from indextts.BigVGAN.models import BigVGAN  # noqa: E402
from indextts.utils.config import Config  # noqa: E402
from indextts.utils.tempo import TempoEngine, fixed_speed, frames, out_len  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempo.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_tempo.py measures on the GPU: none is visible")
DEV, REPS, WARM, SPIN_CYCLES = torch.device("cuda:0"), 9, 2, 2_000_000
SECONDS, N, T = 10, 240000, 938
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return f"{statistics.median(v):.1f}  [{min(v):.1f} .. {max(v):.1f}]"


engine = TempoEngine(DEV)
voc = BigVGAN(Config(weights.reference_config()["bigvgan"]))
voc.load_state_dict(weights.bigvgan_state_dict())
voc.to(DEV).to(torch.float16).remove_weight_norm()
g = torch.Generator().manual_seed(3)
spk = torch.randn(1, 1, 512, generator=g).to(DEV)
base = [torch.from_numpy(R.speechlike(N, seed=100 + r)).to(DEV) for r in range(32)]

say(f"rows of {SECONDS} s ({N} samples at 24 kHz); us, median of {REPS} [min .. max] between device events behind a queued spin kernel; "
    f"vocoder: BigVGAN.forward fp16 over [rows, {T}, 1280] latents, median of 5")
for rows in (1, 32):
    lat = (torch.randn(rows, T, 1280, generator=g) * 0.5).to(DEV).half()
    voc(lat, speaker_embedding=spk)
    torch.cuda.synchronize()
    vt = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        voc(lat, speaker_embedding=spk)
        e1.record()
        torch.cuda.synchronize()
        vt.append(e0.elapsed_time(e1) * 1e3)
    del lat
    say(f"{rows} rows: vocoder {med(vt)}")
    for speed in (0.8, 1.25):
        S = fixed_speed(speed)
        spans = {"search": [], "overlap_add": []}
        real = {k: getattr(natm, k) for k in spans}
        per = {k: [] for k in spans}

        def wrap(name):
            def wrapped(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(SPIN_CYCLES)       # keeps the stream busy while the host enqueues what follows
                e0.record()
                r = real[name](*a)
                e1.record()
                spans[name].append((e0, e1))
                return r
            return wrapped

        for k in spans:
            setattr(natm, k, wrap(k))
        try:
            for rep in range(WARM + REPS):
                for k in spans:
                    spans[k].clear()
                out = engine.process(base[:rows], [S] * rows)
                torch.cuda.synchronize()
                if rep >= WARM:
                    for k in spans:
                        per[k].append(sum(a.elapsed_time(b) for a, b in spans[k]) * 1e3)
        finally:
            for k in spans:
                setattr(natm, k, real[k])
        assert all(int(o.numel()) == out_len(N, S) for o in out)
        both = [a + b for a, b in zip(per["search"], per["overlap_add"])]
        K = frames(N, S)
        say(f"  speed {speed} (S = {S}; {K} frames, {out_len(N, S)} outputs a row): ittm_search {med(per['search'])} "
            f"({statistics.median(per['search']) / (K - 1):.2f} us a frame), ittm_overlap_add {med(per['overlap_add'])}, "
            f"both {med(both)} = {statistics.median(both) / statistics.median(vt):.4f} of the vocoder's time")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
