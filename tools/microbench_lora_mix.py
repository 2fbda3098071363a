#!/usr/bin/env python3
"""What the extra entries of an adapter mix cost, in one process on one box (product library, bf16, 32 rows, graph replay):

  1. per launch: itts_lora_shrink_mix with 1, 2 and 4 entries per row against itts_lora_shrink, in the decode step's form (packed
     operand, packed tail) at K = 1280 and K = 5120, a bank of n = 8 adapters of rank 16 (rp = 16, Kx = 128), the rows' voices
     spread over the bank.  A graph holds LAUNCHES back-to-back launches of one arm (all read the same operand: the A factors
     come from L2 from the second launch on, as they do in a decode step once two rows share a voice); REPEATS timed windows of
     REPLAYS replays per arm, the arms alternating inside every repeat; median and min .. max over the repeats.
  2. per token: the 24-layer engine's graph-replayed decode step (BASELINE config 3 shape: 72-position prompt, 140 tokens, sampling)
     with the bank attached -- rows on adapter ids, rows on one-entry mixes, rows on two-entry mixes -- alternating, ROUNDS rounds.

Appends to $OUT/lora_mix.txt (OUT defaults to out/ under the repository root).  usage: microbench_lora_mix.py [launch] [token]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from indextts import _native as nat  # noqa: E402

torch.set_grad_enabled(False)
parts = sys.argv[1:] or ["launch", "token"]
DEV, T = "cuda", torch.bfloat16
B, N_AD, RANK = 32, 8, 16
LAUNCHES, REPLAYS, REPEATS, ROUNDS = 96, 20, 7, 3
OUT = os.path.join(ROOT, os.environ.get("OUT", "out"))
os.makedirs(OUT, exist_ok=True)
out = open(os.path.join(OUT, "lora_mix.txt"), "a")


def say(line=""):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def mixes(entries):
    """Row b: `entries` voices starting at b's own, equal weights (one entry: weight 1, the id path's result)."""
    return [tuple(sorted(((b + j) % N_AD, 1.0 / entries) for j in range(entries))) for b in range(B)]


say(f"library: {os.environ.get('ITTS_HIP_LIB') or nat.LIB_PATH}")
if "launch" in parts:
    g = torch.Generator().manual_seed(1)
    rp, Kx, Bp = 16, nat.lora_kx(N_AD, 16), nat.packed_rows(B)
    for K in (1280, 5120):
        a_bank = (torch.randn(N_AD, rp, K, generator=g) * 0.05).to(T).to(DEV)
        x = torch.cat([nat.pack_activation((torch.randn(B, K, generator=g)).to(T).to(DEV)), torch.zeros(Bp * Kx, dtype=T, device=DEV)])
        ids = torch.tensor([b % N_AD for b in range(B)], dtype=torch.int32, device=DEV)
        tabs = {e: torch.from_numpy(nat.pack_lora_mix(mixes(e))).to(DEV) for e in (1, 2, 4)}
        arms = {"shrink (ids)": lambda: nat.lora_shrink(x, ids, a_bank, x[Bp * K:], B, K, x_packed=True, u_packed=True)}
        for e in (1, 2, 4):
            arms[f"mix, {e} entr{'y' if e == 1 else 'ies'}"] = \
                lambda e=e: nat.lora_shrink_mix(x, tabs[e], a_bank, x[Bp * K:], B, K, x_packed=True, u_packed=True)
        graphs = {}
        for name, fn in arms.items():
            fn()                                                     # warm-up: code object, first touch
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(LAUNCHES):
                    fn()
            gr.replay()
            torch.cuda.synchronize()
            graphs[name] = gr
        us = {name: [] for name in arms}
        for _ in range(REPEATS):
            for name, gr in graphs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(REPLAYS):
                    gr.replay()
                e.record()
                torch.cuda.synchronize()
                us[name].append(1e3 * s.elapsed_time(e) / (REPLAYS * LAUNCHES))
        say(f"per launch, K = {K}, bf16, {B} rows, n = {N_AD}, rp = {rp}  ({LAUNCHES} launches per graph, {REPLAYS} replays per window, "
            f"{REPEATS} windows per arm, alternating)")
        base = statistics.median(us["shrink (ids)"])
        for name, v in us.items():
            say(f"  {name:16s} median {statistics.median(v):6.2f} us   min {min(v):6.2f}   max {max(v):6.2f}   "
                f"x{statistics.median(v) / base:5.2f} of shrink")
    say()

if "token" in parts:
    import weights  # noqa: E402
    from indextts.gpt.engine import GPTEngine  # noqa: E402
    L, D, P, NEW = 24, 1280, 72, int(os.environ.get("ITTS_TOKENS", "140"))
    gsd = weights.gpt_state_dict(L)
    eng = GPTEngine(gsd, L, D, 20, dtype=T, device=DEV)
    g = torch.Generator().manual_seed(1)
    prefix = torch.randn(B, P, D, generator=g) * 0.1
    pad = torch.zeros(B, dtype=torch.int32)
    sp = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, seed=7)

    def adapters():
        ad = {}
        for i in range(L):
            for name in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"):
                k_in, n_out = gsd[f"gpt.h.{i}.{name}.weight"].shape
                ad[f"gpt.h.{i}.{name}"] = (torch.randn(RANK, k_in, generator=g) * 0.02, torch.randn(n_out, RANK, generator=g) * 0.02)
        return ad
    eng.attach_lora_bank([(adapters(), 2.0) for _ in range(N_AD)])
    voices = {"ids": dict(adapter_ids=[b % N_AD for b in range(B)]), "mix, 1 entry": dict(adapter_mix=mixes(1)),
              "mix, 2 entries": dict(adapter_mix=mixes(2))}
    us = {name: [] for name in voices}

    def run(kw):
        eng.prefill(prefix, pad, NEW + 2, **kw)
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.decode(NEW, sp, force_stop=[NEW - 1] * B)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t) / NEW
    for kw in voices.values():
        run(kw)                                                      # warm-up + capture
    for _ in range(ROUNDS):
        for name, kw in voices.items():
            us[name].append(run(kw))
    say(f"per token: {L} layers, bf16, {B} rows, {P}-position prompt, {NEW} tokens, sampling, bank of n = {N_AD} rank-{RANK} adapters on all "
        f"four targets (96 shrink launches per token); {ROUNDS} rounds, alternating")
    base = statistics.median(us["ids"])
    for name, v in us.items():
        say(f"  {name:16s} median {statistics.median(v):8.1f} us/token   min {min(v):8.1f}   max {max(v):8.1f}   "
            f"{statistics.median(v) - base:+7.1f} us against ids")
    say(f"  graphs held by the engine: {len(eng._graphs)} (one for the id launch, one for the mix launch)")
