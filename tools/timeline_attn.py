#!/usr/bin/env python3
"""Where does a decode-attention launch spend its microseconds?  In-kernel time stamps (diagnostic build only).

Needs libindextts_hip_diag.so (make -C index-tts-lora_amd/csrc diag).  A full-size bf16 engine (32 rows x 20 heads, one
prompt: paged cache, kv_share set -- the arguments of bench.py's flagship step) is prefilled and decodes to three contexts:
the first tokens, mid-utterance (S0 + 70) and the last tokens (S0 + 139).  At each, ONE decode step is captured into a graph
with a distinct stamp area per attention launch (every launch sits behind its QKV' GEMM, as in the token loop) and replayed;
the stamps of the last replay are read back.  Per launch every workgroup's wave 0 recorded (include/indextts_hip_diag.h):
  s_memtime at  0 entry | 1 trip 1 back (pad, pos, skip / share words) | 2 last K / V request issued | 3 first K landed |
                4 last K landed | 5 last V landed | 6 merged (cross-wave barrier passed, output value known) | 7 store issued;
  [12] key slots of the row (ctx - b0), [13] chunks per wave of its first pass, [14] / [15] s_memrealtime at entry / exit.
Printed per context (median over the step's launches of the per-launch median over workgroups, us): the segments, a
workgroup's life, dispatch skew (first to last workgroup entry), kernel span (first entry to last exit).
Read the SHARES, not the lengths: "landed" stamps wait for that request, which forbids overlaps the product kernel has.

    ITTS_HIP_LIB=index-tts-lora_amd/indextts/_lib/libindextts_hip_diag.so python tools/timeline_attn.py [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.setdefault("ITTS_HIP_LIB", os.path.join(ROOT, "index-tts-lora_amd", "indextts", "_lib", "libindextts_hip_diag.so"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEGS = ["trip 1 (query, pad, pos, words, table)", "address + issue K/V requests", "first K lands", "K stream lands",
        "V stream lands (+ scores)", "softmax, PV, merge, barrier", "store"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--tokens", type=int, nargs="*", default=[1, 70, 139])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    import weights
    from indextts import _native as nat
    from indextts.gpt.model import UnifiedVoice
    L = nat.lib()
    L.itts_debug_stamps.restype = ctypes.c_int
    L.itts_debug_stamps.argtypes = [ctypes.c_void_p]
    nat.debug_set(8, 1)                                  # itts_debug_stamps addresses the decode attention from here on
    torch.set_grad_enabled(False)
    dev = "cuda"
    m = UnifiedVoice(**dict(weights.reference_config()["gpt"], layers=args.layers))
    m.load_state_dict(weights.gpt_state_dict(args.layers))
    m.to(dev).to(torch.bfloat16).post_init_gpt2_config(kv_cache=True)
    eng = m.engine
    B, H = args.batch, eng.H
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(20, 61, (B,), generator=g)
    text = torch.full((B, int(lens.max())), 1, dtype=torch.long)
    for i, n in enumerate(lens):
        text[i, : int(n)] = torch.randint(2, 12000, (int(n),), generator=g)
    cond_mel = torch.from_numpy(synth.uniform("bench.cond_mel", (1, 100, 300), -6.0, 2.0)).to(dev)
    conds = m.get_conditioning(cond_mel, None)
    _, emb, mask = m.prepare_gpt_inputs(conds, text.to(dev))
    pad = (mask == 0).sum(1).to(torch.int32)
    sp = dict(do_sample=True, top_p=0.8, top_k=30, temperature=1.0, repetition_penalty=10.0, seed=1)
    max_new = max(args.tokens) + 16
    REPLAYS = 5
    out = {"batch": B, "heads": H, "layers": args.layers, "paged": eng.paged, "segments": SEGS, "contexts": []}
    orig = nat.attn_decode
    for ntok in args.tokens:
        eng.prefill(emb, pad, max_new, shared_rows=int(conds.shape[1]))
        eng.decode(ntok, sp, force_stop=[max_new] * B)       # reach the context (and warm everything up)
        stamps = torch.zeros(args.layers, B * H, 16, dtype=torch.int64, device=dev)
        seen = []

        def wrapped(*a, **k):
            L.itts_debug_stamps(ctypes.c_void_p(stamps[len(seen)].data_ptr()))
            seen.append((k.get("kv_tab") is not None, k.get("kv_share") is not None, k.get("skip_rows") is not None))
            return orig(*a, **k)

        sps = eng._seed_to_state(sp)
        nat.attn_decode = wrapped
        try:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                eng._step_kernels(B, sps)
        finally:
            nat.attn_decode = orig
            L.itts_debug_stamps(None)
        assert len(seen) == args.layers, (len(seen), args.layers)
        for _ in range(REPLAYS):
            gr.replay()
        torch.cuda.synchronize()
        st = stamps.cpu().numpy().astype(np.float64)
        finished = int(eng.finished[:B].sum().item())
        share = int(eng.kv_share.item())
        per = []
        for i in range(args.layers):
            s = st[i]
            live = s[:, 5] > 0                                   # workgroups that ran a key pass (not a skipped row)
            if not live.any():
                continue
            s = s[live]
            rt0, rt1 = s[:, 14], s[:, 15]                        # 100 MHz ticks
            clk = np.median((s[:, 7] - s[:, 0]) / np.maximum(rt1 - rt0, 1.0)) * 100.0   # shader MHz
            seg = [float(np.median((s[:, j] - s[:, j - 1]) / clk)) for j in range(1, 8)]
            per.append(dict(seg=seg, life=float(np.median((s[:, 7] - s[:, 0]) / clk)), skew=float((rt0.max() - rt0.min()) / 100.0),
                            span=float((rt1.max() - rt0.min()) / 100.0), clk=float(clk), keys=s[:, 12], nch=s[:, 13]))
        keys = np.concatenate([d["keys"] for d in per])
        nch = np.concatenate([d["nch"] for d in per]).astype(int)
        med = lambda k: round(float(np.median([d[k] for d in per])), 2)   # noqa: E731
        out["contexts"].append({
            "tokens_decoded": ntok + REPLAYS, "cache_position": int(eng.state[1].item()), "finished_rows": finished,
            "args": {"paged": seen[0][0], "kv_share": seen[0][1], "skip_rows": seen[0][2], "share_word_C": share & 255},
            "key_slots_per_row": {"min": int(keys.min()), "median": int(np.median(keys)), "max": int(keys.max())},
            "chunks_per_wave": {str(v): int((nch == v).sum()) for v in sorted(set(nch.tolist()))},
            "segments_us": {name: round(float(np.median([d["seg"][j] for d in per])), 2) for j, name in enumerate(SEGS)},
            "wg_median_life_us": med("life"), "dispatch_skew_us": med("skew"), "kernel_span_us": med("span"),
            "clock_mhz": round(med("clk"), 0)})
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
