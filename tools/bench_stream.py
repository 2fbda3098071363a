#!/usr/bin/env python3
"""Latency of streaming synthesis: one utterance of 140 codes (force_stop), 24 layers, bf16 GPT / fp16 vocoder, through
IndexTTS.stream_utterance in chunks of 16 / 32 / 64 tokens against IndexTTS.infer_batch (one row), alternating, in one process.
Host clock around work that ends in a device synchronise: a chunk counts as delivered when its samples are on the host.  Each
variant is warmed twice (graph capture, prompt features), then the median (min) of `reps` runs is reported.
profiles/stream_latency.txt is this tool's output.
usage: bench_stream.py [reps] [layers]"""
import os
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

torch.set_grad_enabled(False)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 24
STOP, LIMIT, CHUNKS = 140, 192, (16, 32, 64)
GEN = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1)

if not torch.cuda.is_available():
    sys.exit("bench_stream.py measures on the GPU: none is visible")
cfg = weights.reference_config()
cfg["gpt"]["layers"] = layers
tts = IndexTTS.from_weights(cfg, weights.gpt_state_dict(layers), weights.bigvgan_state_dict(), device="cuda:0",
                            precision_config={"gpt": "bf16", "vocoder": "fp16"})
cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to("cuda")
text = torch.from_numpy(np.random.default_rng(11).integers(2, 12000, size=40)).to(torch.int32)
left, right = tts.bigvgan.receptive_halo()


def whole():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wav = tts.infer_batch(cond_mel, [text], max_mel_tokens=LIMIT, force_stop=[STOP], seed=5, **GEN)[0].cpu()
    return 1e3 * (time.perf_counter() - t0), wav


def streamed(chunk):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    at, out = [], []
    for pcm in tts.stream_utterance(cond_mel, text, chunk_tokens=chunk, max_mel_tokens=LIMIT, seed=5, force_stop=[STOP], **GEN):
        out.append(pcm.cpu())
        at.append(1e3 * (time.perf_counter() - t0))
    return at, torch.cat(out)


def stat(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:8.2f} ms ({v[0]:.2f})"


for _ in range(2):
    whole()
    for c in CHUNKS:
        streamed(c)
t_whole = {c: [] for c in CHUNKS}
first, last, n_chunks, rms = ({c: [] for c in CHUNKS} for _ in range(4))
for _ in range(reps):
    for c in CHUNKS:                      # the two paths alternate, so a drift of the machine touches both alike
        ms, ref = whole()
        t_whole[c].append(ms)
        at, wav = streamed(c)
        first[c].append(at[0])
        last[c].append(at[-1])
        n_chunks[c] = len(at)
        rms[c] = ((wav - ref) / 32767.0).pow(2).mean().sqrt().item() if wav.shape == ref.shape else float("nan")
torch.cuda.synchronize()
print(f"stream latency | {layers} layers, bf16 GPT, fp16 vocoder, 1 utterance of {STOP} codes ({STOP * 1024 / 24000:.2f} s of audio), "
      f"text of {text.numel()} tokens, halo (left, right) = ({left}, {right}) frames; median (min) of {reps}, host clock to samples on the host")
all_whole = [v for c in CHUNKS for v in t_whole[c]]
print(f"stream latency | infer_batch, whole utterance (first audio = all audio) | {stat(all_whole)}")
for c in CHUNKS:
    w = sorted(t_whole[c])[len(t_whole[c]) // 2]
    l = sorted(last[c])[len(last[c]) // 2]
    print(f"stream latency | chunks of {c:2d} tokens | first chunk {stat(first[c])}  last chunk {stat(last[c])}  chunks = {n_chunks[c]}  "
          f"total / infer_batch = {l / w:.3f}  waveform rms vs infer_batch = {rms[c]:.2e}")
