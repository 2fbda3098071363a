#!/usr/bin/env python3
"""Conditioner time for N distinct prompts, batched (ConditionerEngine.batch: one pass of 72 launches) against looped (N
single-prompt passes), both as graph replays in one process, timed with events around the replays; and the spread of the batched
latents against the single-prompt engine's.  profiles/prompt_batch.txt is this tool's output.
usage: prompt_batch_time.py [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import synth  # noqa: E402
import weights  # noqa: E402
from indextts.gpt.model import UnifiedVoice  # noqa: E402

torch.set_grad_enabled(False)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
m = UnifiedVoice(**dict(weights.reference_config()["gpt"], layers=2))
m.load_state_dict(weights.gpt_state_dict(2))
m.to("cuda").to(torch.bfloat16)
eng = m.conditioner()


def mels_of(frames):
    return [torch.from_numpy(synth.uniform(f"in.cond_mel.{i}", (1, 100, T), -6.0, 2.0)).to("cuda")[0].t().contiguous()
            for i, T in enumerate(frames)]


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def replay_ms(g, n):
    for _ in range(3):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(n):
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


print("spread: max |ConditionerEngine.batch - single-prompt engine| per prompt (fp16 kernels, latents of RMS ~1)")
frames = [35, 36, 67, 120, 437]
mels = mels_of(frames)
got = eng.batch(mels).clone()
worst = 0.0
for i, x in enumerate(mels):
    e = (got[i] - eng(x)).abs().max().item()
    worst = max(worst, e)
    print(f"  frames {frames[i]:4d}: {e:.3e}")
print(f"  max over the five prompts: {worst:.3e}")

print(f"conditioner time, graph replays, events around each replay, median (min) of {reps}; prompts of 240 .. 360 frames")
for n in (1, 8, 32):
    fr = [240 + (37 * i) % 121 for i in range(n)]
    ms = mels_of(fr)
    gb, _ = graphed(lambda: eng.batch(ms))
    gl, _ = graphed(lambda: [eng(x).clone() for x in ms])
    tb, tl = replay_ms(gb, reps), replay_ms(gl, reps)
    print(f"  N = {n:2d} ({sum((T - 3) // 2 + 1 for T in fr)} rows): batched {tb[0]:7.3f} ms ({tb[1]:.3f})   looped {tl[0]:7.3f} ms ({tl[1]:.3f})"
          f"   {tl[0] / tb[0]:.2f} x")
    eng.forget()
    # what IndexTTS's prompt-list path runs: the eager pass over views of [1, 100, T] mels, unretained buffers (second call on: the
    # set is cached), timed on the host around a synchronised call
    views = [x.t().contiguous()[None][0].t() for x in ms]
    ts = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.batch(views, retain=False).clone()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"           eager, unretained (the prompt-list path): first call {ts[0]:7.3f} ms, then median {sorted(ts[1:])[2]:7.3f} ms")
    eng.forget()
