#!/usr/bin/env python3
"""The two kernel forms of the cached-prefix append attention (itts_attn_prefill_shared with pre_row0 = NULL) at a stream's chunk
shapes: E elements of `rows` new rows each behind `pre` cached keys, 20 heads, bf16.  Smax selects the form (<= 128: the
16-query tile; Smax may exceed the longest element, so Smax = 129 runs the same work through the 64-query tile).  Device events
around `iters` back-to-back launches after a warm-up, forms alternating, median of 9 (per launch, in microseconds).
usage: bench_attn_append.py [iters]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from indextts import _native as nat  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
H, smax, dev, T = 20, 1024, "cuda", torch.bfloat16
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731


def per_launch(E, rows, pre, Smax):
    qkv = torch.randn(E * rows, 3 * H * 64, device=dev).to(T)
    out = torch.empty(E * rows, H * 64, device=dev, dtype=T)
    kc, vc = (torch.randn(E, H, smax, 64, device=dev).to(T) for _ in range(2))
    args = (i32([rows * e for e in range(E + 1)]), i32([pre] * E), i32(list(range(E))), i32([pre] * E), E, Smax, H, smax)
    for _ in range(20):
        nat.attn_prefill_append(qkv, out, kc, vc, *args)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        nat.attn_prefill_append(qkv, out, kc, vc, *args)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters, nat.last_kernel()


for E, rows, pre in ((1, 16, 200), (1, 16, 560), (8, 16, 560), (32, 16, 560), (1, 64, 560), (8, 64, 560)):
    res = {16: [], 129: []}
    for _ in range(9):
        for Smax in (max(rows, 16), 129):
            us, name = per_launch(E, rows, pre, Smax)
            res[16 if Smax < 129 else 129].append(us)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    print(f"attn append forms | E = {E:2d} elements x {rows} new rows behind {pre} keys, H = 20, bf16 | attn_append<16> {med[16]:7.2f} us  "
          f"attn_append<64> {med[129]:7.2f} us  <16> / <64> = {med[16] / med[129]:.3f}")
