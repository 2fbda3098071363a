#!/usr/bin/env python3
"""Latency of streaming synthesis: one utterance of 140 codes (force_stop), 24 layers, bf16 GPT / fp16 vocoder, through
IndexTTS.stream_utterance in chunks of 16 / 32 / 64 tokens against IndexTTS.infer_batch (one row), alternating, in one process.
Host clock around work that ends in a device synchronise: a chunk counts as delivered when its samples are on the host.  Each
variant is warmed twice (graph capture, prompt features), then the median (min) of `reps` runs is reported.
profiles/stream_latency.txt is this tool's output.
--rows N: N utterances (texts of 40 tokens, stops spread from 140 down to 100 codes) through ONE IndexTTS.stream_batch against N
sequential stream_utterance calls and against one infer_batch of the N rows, alternating in one process, at --chunk tokens:
the time to the first chunk of row 0 and to the last chunk of the last row.  profiles/stream_batch_latency.txt is that output.
--queue N --slots S: N utterances of mixed lengths (BASELINE config 4's: texts of U{8..100} tokens, stops after U{40..400} codes, seed 3)
through IndexTTS.stream_queue with S slots, against stream_batch in ceil(N / S) static batches of S and against infer_queue on
the same queue, alternating in one process: the time to every utterance's first chunk (median and worst over the utterances)
and to the last chunk of the queue.  profiles/stream_queue_latency.txt is that output.
--latent-cache: latent_cache=False (the latent pass repeated over all k codes per boundary) against latent_cache=True (the incremental
pass, GPTEngine.latent_append), alternating in one process: first and last chunk of the one-utterance table (chunks of 16 / 32 / 64), of
stream_batch with --rows N (stops spread from --stop down to --stop - 40) or of stream_queue with --queue N --slots S; then one run of
each with the latent pass timed per boundary (synchronised around it, so those runs are not the ones the chunk times come from).
profiles/stream_latent_cache.txt is that output.
usage: bench_stream.py [reps] [layers] [--rows N] [--chunk C] [--queue N --slots S] [--latent-cache [--stop T]]"""
import argparse
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
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=9)
ap.add_argument("layers", nargs="?", type=int, default=24)
ap.add_argument("--rows", type=int, default=0, help="N utterances through one stream_batch (0: the one-utterance table)")
ap.add_argument("--chunk", type=int, default=32, help="chunk_tokens of the --rows table")
ap.add_argument("--queue", type=int, default=0, help="N utterances of mixed lengths through stream_queue (0: off)")
ap.add_argument("--slots", type=int, default=32, help="decode slots of the --queue table")
ap.add_argument("--latent-cache", action="store_true", help="latent_cache=False against latent_cache=True on the chosen table")
ap.add_argument("--stop", type=int, default=140, help="codes of the longest utterance of the --latent-cache tables")
args = ap.parse_args()
reps, layers = args.reps, args.layers
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


def rows_table(N, chunk):
    """N utterances: one stream_batch | N sequential stream_utterance | one infer_batch, alternating."""
    rng = np.random.default_rng(12)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=40)).to(torch.int32) for _ in range(N)]
    stops = [STOP - (40 * i) // max(N - 1, 1) for i in range(N)]

    def batch_whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wavs = [w.cpu() for w in tts.infer_batch(cond_mel, texts, max_mel_tokens=LIMIT, force_stop=stops, seed=5, **GEN)]
        return 1e3 * (time.perf_counter() - t0), wavs

    def batch_streamed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first0, n_ev, out = None, 0, [[] for _ in range(N)]
        for row, pcm, _ in tts.stream_batch(cond_mel, texts, chunk_tokens=chunk, max_mel_tokens=LIMIT, seed=5, force_stop=stops, **GEN):
            out[row].append(pcm.cpu())
            n_ev += 1
            if row == 0 and first0 is None:
                first0 = 1e3 * (time.perf_counter() - t0)
        return first0, 1e3 * (time.perf_counter() - t0), n_ev, [torch.cat(o) for o in out]

    def one_by_one():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first0 = None
        for i in range(N):
            for pcm in tts.stream_utterance(cond_mel, texts[i], chunk_tokens=chunk, max_mel_tokens=LIMIT, seed=5, force_stop=[stops[i]], **GEN):
                pcm.cpu()
                if first0 is None:
                    first0 = 1e3 * (time.perf_counter() - t0)
        return first0, 1e3 * (time.perf_counter() - t0)

    for _ in range(2):
        batch_whole(), batch_streamed(), one_by_one()
    t_w, b_first, b_last, s_first, s_last = [], [], [], [], []
    for _ in range(reps):                 # the three paths alternate, so a drift of the machine touches all alike
        ms, ref = batch_whole()
        t_w.append(ms)
        f, l, n_ev, wavs = batch_streamed()
        b_first.append(f)
        b_last.append(l)
        f, l = one_by_one()
        s_first.append(f)
        s_last.append(l)
    rms = max(((a - b) / 32767.0).pow(2).mean().sqrt().item() if a.shape == b.shape else float("nan") for a, b in zip(wavs, ref))
    audio = sum(stops) * 1024 / 24000
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    tag = f"stream batch latency | {N} rows, chunks of {chunk}"
    print(f"stream batch latency | {layers} layers, bf16 GPT, fp16 vocoder, {N} utterances of {stops} codes ({audio:.2f} s of audio), texts of 40 "
          f"tokens, chunks of {chunk} tokens, halo (left, right) = ({left}, {right}) frames; median (min) of {reps}, host clock to samples on the host")
    print(f"{tag} | infer_batch, whole utterances (first audio = all audio)  | {stat(t_w)}  {audio / med(t_w) * 1e3:7.1f} audio-s/s")
    print(f"{tag} | stream_batch, one token loop                             | first chunk of row 0 {stat(b_first)}  last chunk of the last row "
          f"{stat(b_last)}  {audio / med(b_last) * 1e3:7.1f} audio-s/s  events = {n_ev}  worst row rms vs infer_batch = {rms:.2e}")
    print(f"{tag} | {N} x stream_utterance, one after another{' ' * (21 - len(str(N)))}| first chunk of row 0 {stat(s_first)}  last chunk of the last row "
          f"{stat(s_last)}  {audio / med(s_last) * 1e3:7.1f} audio-s/s")
    print(f"{tag} | last chunk: stream_batch / sequential = {med(b_last) / med(s_last):.3f}, stream_batch / infer_batch = {med(b_last) / med(t_w):.3f}; "
          f"first chunk of row 0: stream_batch / sequential = {med(b_first) / med(s_first):.3f}")


def queue_table(N, S, chunk):
    """N utterances of mixed lengths: stream_queue(slots=S) | stream_batch in static batches of S | infer_queue, alternating."""
    rng = np.random.default_rng(3)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=int(n))).to(torch.int32) for n in rng.integers(8, 101, size=N)]
    stops = [int(v) for v in rng.integers(40, 401, size=N)]
    kw = dict(max_mel_tokens=416, seed=5, **GEN)

    def stamp(events, t0):
        first, n_ev = {}, 0
        for utt, pcm, _ in events:
            pcm.cpu()
            n_ev += 1
            first.setdefault(utt, 1e3 * (time.perf_counter() - t0))
        return first, 1e3 * (time.perf_counter() - t0), n_ev

    def queued():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        return stamp(tts.stream_queue(cond_mel, texts, slots=S, chunk_tokens=chunk, force_stop=stops, **kw), t0)

    def static():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first, n_ev = {}, 0
        for s0 in range(0, N, S):
            f, last, n = stamp(((s0 + r, p, l) for r, p, l in tts.stream_batch(cond_mel, texts[s0: s0 + S], chunk_tokens=chunk,
                                                                              force_stop=stops[s0: s0 + S], **kw)), t0)
            first.update(f)
            n_ev += n
        return first, last, n_ev

    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for w in tts.infer_queue(cond_mel, texts, slots=S, check_every=chunk, force_stop=stops, **kw):
            w.cpu()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(2):
        queued(), static(), whole()
    res = {"queue": [], "static": []}
    t_whole = []
    for _ in range(reps):                 # the three paths alternate, so a drift of the machine touches all alike
        res["queue"].append(queued())
        res["static"].append(static())
        t_whole.append(whole())
    audio = sum(stops) * 1024 / 24000
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    tag = f"stream queue latency | {N} utterances, {S} slots, chunks of {chunk}"
    print(f"stream queue latency | {layers} layers, bf16 GPT, fp16 vocoder, {N} utterances of 40 .. 400 codes ({audio:.2f} s of audio, {sum(stops)} "
          f"codes), texts of 8 .. 100 tokens, {S} slots, chunks of {chunk} tokens, halo (left, right) = ({left}, {right}) frames; median (min) of {reps}, "
          f"host clock to samples on the host")
    print(f"{tag} | infer_queue, whole utterances (first audio = all audio) | {stat(t_whole)}  {audio / med(t_whole) * 1e3:7.1f} audio-s/s")
    for name, label in (("queue", "stream_queue, one refilled loop          "), ("static", f"stream_batch, static batches of {S:<9d}")):
        runs = res[name]
        f_med = [med(list(f.values())) for f, _, _ in runs]
        f_max = [max(f.values()) for f, _, _ in runs]
        last = [l for _, l, _ in runs]
        print(f"{tag} | {label} | first chunk of an utterance: median {stat(f_med)}  worst {stat(f_max)}  last chunk of the queue {stat(last)}  "
              f"{audio / med(last) * 1e3:7.1f} audio-s/s  events = {runs[-1][2]}")
    ql, sl = med([l for _, l, _ in res["queue"]]), med([l for _, l, _ in res["static"]])
    print(f"{tag} | last chunk: stream_queue / static stream_batch = {ql / sl:.3f}, stream_queue / infer_queue = {ql / med(t_whole):.3f}")


def latent_cache_table():
    """latent_cache False | True, alternating: (first, last) chunk times per form, then the latent pass per boundary."""
    rng = np.random.default_rng(12)
    stop, limit = args.stop, args.stop + 52
    if args.queue > 0:
        r3 = np.random.default_rng(3)
        texts = [torch.from_numpy(r3.integers(2, 12000, size=int(n))).to(torch.int32) for n in r3.integers(8, 101, size=args.queue)]
        stops = [int(v) for v in r3.integers(40, 401, size=args.queue)]
        forms = [(f"stream_queue, {args.queue} utterances of 40 .. 400 codes, {args.slots} slots, chunks of {args.chunk}",
                  lambda lc: tts.stream_queue(cond_mel, texts, slots=args.slots, chunk_tokens=args.chunk, force_stop=stops, max_mel_tokens=416,
                                              seed=5, latent_cache=lc, **GEN))]
    elif args.rows > 0:
        N = args.rows
        texts = [torch.from_numpy(rng.integers(2, 12000, size=40)).to(torch.int32) for _ in range(N)]
        stops = [stop - (40 * i) // max(N - 1, 1) for i in range(N)]
        forms = [(f"stream_batch, {N} rows of {stops[0]} .. {stops[-1]} codes, chunks of {args.chunk}",
                  lambda lc: tts.stream_batch(cond_mel, texts, chunk_tokens=args.chunk, max_mel_tokens=limit, seed=5, force_stop=stops,
                                              latent_cache=lc, **GEN))]
    else:
        forms = [(f"stream_utterance, {stop} codes, chunks of {c:2d}",
                  lambda lc, c=c: ((0, p, False) for p in tts.stream_utterance(cond_mel, text, chunk_tokens=c, max_mel_tokens=limit, seed=5,
                                                                              force_stop=[stop], latent_cache=lc, **GEN))) for c in CHUNKS]

    def run(form, lc):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at = []
        for _, pcm, _ in form(lc):
            if pcm.numel():
                pcm.cpu()
                at.append(1e3 * (time.perf_counter() - t0))
        return at[0], at[-1]

    def timed(form, lc):
        """one run with the latent pass wrapped: [(rows the pass was asked for, ms)] per boundary"""
        name, out = ("_latents_incremental", []) if lc else ("_latents", [])
        real = getattr(tts, name)

        def wrapped(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = real(*a, **k)
            torch.cuda.synchronize()
            out.append((sum(int(x.shape[0]) for x in r), 1e3 * (time.perf_counter() - t0)))
            return r
        setattr(tts, name, wrapped)
        try:
            run(form, lc)
        finally:
            delattr(tts, name)
        return out

    print(f"stream latent cache | {layers} layers, bf16 GPT, fp16 vocoder, text(s) of 40 tokens unless said, halo (left, right) = ({left}, {right}) "
          f"frames; median (min) of {reps}, host clock to samples on the host; latent_cache False and True alternate in one process")
    for label, form in forms:
        for _ in range(2):
            run(form, False), run(form, True)
        res = {False: [], True: []}
        for _ in range(reps):
            for lc in (False, True):
                res[lc].append(run(form, lc))
        med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
        for lc in (False, True):
            print(f"stream latent cache | {label} | latent_cache={lc!s:5} | first chunk {stat([f for f, _ in res[lc]])}  last chunk "
                  f"{stat([l for _, l in res[lc]])}")
        print(f"stream latent cache | {label} | last chunk True / False = {med([l for _, l in res[True]]) / med([l for _, l in res[False]]):.3f}  "
              f"first chunk True / False = {med([f for f, _ in res[True]]) / med([f for f, _ in res[False]]):.3f}")
        for lc in (False, True):
            per = timed(form, lc)
            print(f"stream latent cache | {label} | latent_cache={lc!s:5} | latent pass per boundary, (frames held by the emitting rows: ms) = "
                  + "  ".join(f"{k}: {ms:.2f}" for k, ms in per[:24]) + f"  | sum = {sum(ms for _, ms in per):.1f} ms over {len(per)} passes")


if args.latent_cache:
    latent_cache_table()
    torch.cuda.synchronize()
    sys.exit(0)

if args.queue > 0:
    queue_table(args.queue, args.slots, args.chunk)
    torch.cuda.synchronize()
    sys.exit(0)

if args.rows > 0:
    rows_table(args.rows, args.chunk)
    torch.cuda.synchronize()
    sys.exit(0)

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
