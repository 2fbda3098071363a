#!/usr/bin/env python3
"""The speaking rate measured: 1 and 32 utterances of 10 s (fp32 at 24 kHz on the device, speech-like:
tests/tempo_refs.speechlike) at the speeds 0.8 and 1.25 -> the two launches of TempoEngine.process, ittm_search and
ittm_overlap_add, each between two device events behind a queued spin kernel (the host's enqueueing is not in the span);
median of 9 after two warm-up rounds.  Beside them, in the same run: BigVGAN.forward (fp16, the synthetic weights of
tests/weights.py) over the latents of the same rows -- 938 frames a row -- between device events, median of 5 after one warm-up.
ittm_search walks a row's chain in ONE workgroup: its time is that of the longest row, whatever the batch, up to one row per CU.
No threshold is fixed in advance: the output is the record.  Writes profiles/tempo.txt.
--pitch SEMITONES measures the pitch shift instead, on the same rows: ittr_resample_ratio alone between
device events behind the spin kernel, median of 7, with the bytes it moves (the samples it reads and writes once, and the table a
workgroup) against that time; the three launches of TempoEngine.shift(pitch=SEMITONES) and the whole call between device events,
against TempoEngine.process at speed 0.8 (speed= alone) measured the same way; and the kernel's largest error / bound on row 0
against tempo.resample_ratio_ref.  Writes profiles/pitch.txt.
usage: bench_tempo.py [--pitch SEMITONES] [--out FILE]"""
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
from indextts import _native_pitch as natr  # noqa: E402
from indextts import _native_tempo as natm  # noqa: E402
from indextts.BigVGAN.models import BigVGAN  # noqa: E402
from indextts.utils.config import Config  # noqa: E402
from indextts.utils.tempo import TempoEngine, cutoff_of, fixed_speed, frames, out_len, pitch_plan, ratio_table, resample_ratio_ref  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--pitch", type=float, default=None, metavar="SEMITONES")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "tempo.txt" if args.pitch is None else "pitch.txt")
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


def write_out():
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def timed(mods, call, reps, warm):
    """call() `warm + reps` times with every (module, name) of mods between two device events behind a queued spin kernel, and the
    whole call between two more: ({name: [us a round]}, [us a round of the whole call])."""
    spans = {name: [] for _, name in mods}
    real = {name: getattr(mod, name) for mod, name in mods}
    per, whole = {name: [] for name in spans}, []

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

    for rep in range(2 * (warm + reps)):
        bare = rep >= warm + reps                # the second half: the whole call, without the spin kernels and inner events
        for mod, name in mods:
            setattr(mod, name, real[name] if bare else wrap(name))
            spans[name].clear()
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
        finally:
            for mod, name in mods:
                setattr(mod, name, real[name])
        if bare and rep >= 2 * warm + reps:
            whole.append(e0.elapsed_time(e1) * 1e3)
        elif not bare and rep >= warm:
            for name in spans:
                per[name].append(sum(a.elapsed_time(b) for a, b in spans[name]) * 1e3)
    return per, whole


engine = TempoEngine(DEV)
if args.pitch is not None:
    PREPS = 7
    rate, step, resampled = pitch_plan(args.pitch)
    S = fixed_speed(rate)
    mid = out_len(N, S)
    say(f"tools/bench_tempo.py --pitch {args.pitch:g}: rows of {SECONDS} s ({N} samples at 24 kHz), p = {step / 2 ** 32:.6f} (step {step}, cutoff "
        f"{cutoff_of(step)} / 65536), WSOLA at S = {S} -> {mid} samples a row, resampled to {resampled(mid)}; us, median of {PREPS} "
        f"[min .. max] between device events behind a queued spin kernel; `whole call`: the call between two device events, no spin kernel")
    for rows in (1, 32):
        base = [torch.from_numpy(R.speechlike(N, seed=100 + r)).to(DEV) for r in range(rows)]
        mods = [(natm, "search"), (natm, "overlap_add"), (natr, "resample_ratio")]
        per, whole = timed(mods, lambda: engine.shift(base, pitch=args.pitch), PREPS, WARM)
        out = engine.shift(base, pitch=args.pitch)
        assert all(int(o.numel()) == resampled(mid) for o in out)
        moved = rows * 4 * (mid + resampled(mid))
        tiles = rows * ((resampled(mid) + natr.TILE - 1) // natr.TILE)
        t_r = statistics.median(per["resample_ratio"])
        three = [a + b + c for a, b, c in zip(per["search"], per["overlap_add"], per["resample_ratio"])]
        say(f"{rows} rows: ittr_resample_ratio {med(per['resample_ratio'])}: {moved} bytes of samples read and written once = "
            f"{moved / t_r / 1e3:.1f} GB/s ({tiles} workgroups, each also stages the table: {tiles * 4 * natr.TABLE} bytes from cache)")
        say(f"  shift(pitch={args.pitch:g}): ittm_search {med(per['search'])}, ittm_overlap_add {med(per['overlap_add'])}, the three launches "
            f"{med(three)}; whole call {med(whole)}")
        S8 = fixed_speed(0.8)
        per8, whole8 = timed(mods[:2], lambda: engine.process(base, [S8] * rows), PREPS, WARM)
        two = [a + b for a, b in zip(per8["search"], per8["overlap_add"])]
        say(f"  speed=0.8 alone (S = {S8}): ittm_search {med(per8['search'])}, ittm_overlap_add {med(per8['overlap_add'])}, the two launches "
            f"{med(two)}; whole call {med(whole8)}")
        say(f"  the three launches / the two: {statistics.median(three) / statistics.median(two):.3f}; whole call / whole call: "
            f"{statistics.median(whole) / statistics.median(whole8):.3f}")
    x = engine.process(base[:1], [S])[0]
    got = engine.resample([x], [step])[0].cpu().numpy().astype("float64")
    xh = x.cpu().numpy()
    want, mass = resample_ratio_ref(xh, step, detail=True)
    g = ratio_table().numpy().astype("float64")
    c, u = 65536.0 / cutoff_of(step), 2.0 ** -24
    bound = (2 * natr.HW * c + 3) * u * mass + float(abs(xh).max()) * (2 * natr.HW * c + 1) * u * float(abs(g[1:] - g[:-1]).max()) / c
    say(f"row 0 after WSOLA ({xh.size} samples, |x| up to {abs(xh).max():.0f}) against resample_ratio_ref: largest error / bound "
        f"{float((abs(got - want) / bound).max()):.3f} (the bound of tests/test_pitch_kernels_gpu.py)")
    write_out()
    sys.exit(0)
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

write_out()
