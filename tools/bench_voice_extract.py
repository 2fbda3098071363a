#!/usr/bin/env python3
"""Voice extraction measured at full size: 24 layers, D = 1280, the 96 target matrices of a base held in
fp16 (entries 0.02 N(0,1)) and a merged fp16 checkpoint of a rank-4 and of a rank-16 voice (refill_voices.make_factors).
(a) Wall time of one extraction (voice_extract.extract over DeviceDelta: per target two uploads, four ittv_delta_project launches,
    QR / SVD of c-wide matrices on the host) against the same algorithm in plain torch, written here: the same uploads and the same
    host steps, but the difference materialised in fp32 on the device and four torch.matmul.  Same process, alternating, median of
    `reps`; both must find the same ranks.
(b) Per target shape and op: the launch alone between two events, the NOMINAL bytes 2 K N (element size) -- what the two images
    hold; no counter is read, so bytes fetched are not measured -- and GB/s of that figure, beside torch.matmul on the materialised
    fp32 difference (which reads 4 K N bytes, after a pass that wrote them).  By the kernel's code every weight element is
    requested once, except that lanes past the end of a reduction piece (N not a multiple of 32; column tiles past N) request the
    piece's first elements again and use zeros; at these shapes no lane is past an end.
No threshold is set: the output is the record.  The tool writes sections (a) and (b) of profiles/voice_extract.txt and keeps what
the file holds from its line "(c) ..." on: the engine-parity line that tests/test_voice_extract_gpu.py prints under `-s`, and the
reading of the numbers, both put there by hand.
usage: bench_voice_extract.py [reps] [layers] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from indextts import _native_voice as natv  # noqa: E402
from indextts.gpt import voice_extract  # noqa: E402
from refill_voices import TARGETS, make_factors, merged_state  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=3)
ap.add_argument("layers", nargs="?", type=int, default=24)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_extract.txt"))
args = ap.parse_args()
reps, layers = max(1, args.reps), args.layers
if not torch.cuda.is_available():
    sys.exit("bench_voice_extract.py measures on the GPU: none is visible")
DEV, D = torch.device("cuda:0"), 1280
SHAPES = {"attn.c_attn": (D, 3 * D), "attn.c_proj": (D, D), "mlp.c_fc": (D, 4 * D), "mlp.c_proj": (4 * D, D)}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


g = torch.Generator().manual_seed(1)
base = {f"gpt.h.{i}.{n}.weight": (torch.randn(*SHAPES[n], generator=g) * 0.02).half() for i in range(layers) for n in TARGETS}


class TorchDelta:
    """The plain-torch form: the same uploads, the difference written out in fp32, torch.matmul."""

    def __init__(self, device):
        self.device = device

    def __call__(self, key, wb, wt):
        delta = wt.to(self.device).float() - wb.to(self.device).float()

        def project(x, trans):
            return torch.matmul(delta.t() if trans else delta, x.to(self.device, torch.float32))
        return project


def wall(make, tuned):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ad, _, rep = voice_extract.extract(base, tuned, layers, make, max_rank=16)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, rep


say(f"voice extraction: {layers} layers, D = {D}, {len(base)} targets, base and checkpoint fp16 "
    f"({sum(v.numel() for v in base.values()) * 2 / 1e9:.2f} GB each), max_rank 16 (c = 32), {torch.cuda.get_device_name(0)}")
say("(a) wall time of one extraction, s: median (min) of %d, alternating" % reps)
dev_make, torch_make = voice_extract.DeviceDelta(DEV), TorchDelta(DEV)
for rank, sc in ((4, 2.0), (16, 0.5)):
    bank = make_factors(base, (rank,), (sc,), layers=layers, seed=3)
    tuned = {k: v.half() for k, v in merged_state(base, bank, {0: 1.0}).items()}
    wall(dev_make, tuned), wall(torch_make, tuned)                                   # warm-up: allocator, library loads
    td, tt = [], []
    for _ in range(reps):
        a, rep_d = wall(dev_make, tuned)
        b, rep_t = wall(torch_make, tuned)
        td.append(a), tt.append(b)
    assert all(rep_d[k]["r"] == rep_t[k]["r"] == rank for k in rep_d) and len(rep_d) == len(base)
    worst = min(r["ratio"] for r in rep_d.values())
    say(f"    r = {rank:2d}: ittv_delta_project {statistics.median(td):.3f} ({min(td):.3f})   torch (fp32 difference + matmul) "
        f"{statistics.median(tt):.3f} ({min(tt):.3f})   ranks found {rank} on all {len(rep_d)} targets, smallest sigma_r / sigma_r+1 {worst:.0f}")
    del tuned, bank

say("(b) one launch, us: median of 20 between events (c = 32, fp16 - fp16); MB = 2 K N 2 bytes, nominal (what the two images hold: "
    "no counter was read); GB/s = that figure / kernel time")
say("    target        K     N   op   nominal MB   kernel us   GB/s   torch.matmul on fp32 difference us")
ws = natv.delta_workspace(DEV)


def timed(fn, n=20):
    fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


for name, (K, N) in SHAPES.items():
    wb = base[f"gpt.h.0.{name}.weight"].to(DEV)
    wt = (wb.float() + torch.randn(K, N, device=DEV) * 0.0016).half()
    delta = wt.float() - wb.float()
    for trans in (False, True):
        x = torch.randn(K if trans else N, 32, device=DEV)
        out = torch.empty(N if trans else K, 32, device=DEV)
        tk = timed(lambda: natv.delta_project(wt, wb, x, trans, ws, out=out))
        tm = timed(lambda: torch.matmul(delta.t() if trans else delta, x, out=out))
        nbytes = 2 * K * N * 2
        say(f"    {name:12s} {K:5d} {N:5d}   {'D^T' if trans else 'D  '}  {nbytes / 1e6:10.1f}   {tk:9.1f}   {nbytes / tk / 1e3:6.0f}   {tm:9.1f}")
kept = []
if os.path.exists(args.out):                                    # sections (c) on are not this tool's: they stay
    old = open(args.out).read().splitlines()
    at = next((i for i, ln in enumerate(old) if ln.startswith("(c) ")), None)
    kept = [] if at is None else old[at:]
lines += kept
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
