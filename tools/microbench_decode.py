#!/usr/bin/env python3
"""Slot time of each decode-step kernel inside a replayed CUDA graph (MI355X; writes gpurun_out/microbench.txt).

Each experiment captures `reps` launches cycling through 24 layers' worth of distinct weights (so the weight stream is
real HBM traffic, not L2 hits), replays the graph a few times and reports microseconds per launch.
  --w8: only the FP8-weight comparison (w8_report: the "fold" step's five GEMMs and a 24-layer engine, FP8 against bf16).
  --kv8: only the FP8 KV cache comparison (kv8_report: the decode attention per launch at config 3's contexts, paged 16-bit cache
         against the E4M3 cache, and a 24-layer engine's us per token with both caches, bf16 and FP8 weights)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import os as _os
_os.environ.setdefault("ITTS_HIP_LIB", _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "index-tts-lora_amd", "indextts", "_lib", "libindextts_hip_diag.so"))  # tuning knobs live in the diagnostic build
import torch  # noqa: E402

from indextts import _native as nat  # noqa: E402

dev = "cuda"
T = torch.bfloat16
B, D, H, L = 32, 1280, 20, 24
out = open(os.path.join(ROOT, "gpurun_out", "microbench.txt"), "a")


def log(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def timed_graph(fn, reps_in_graph, replays=20):
    fn()  # warm-up (loads code objects)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * reps_in_graph)


def rand_w(K, N):
    return nat.pack_weight((torch.randn(K, N, device=dev) * 0.02).to(T))


def w8_report():
    """--w8: the five decode-step GEMMs of the "fold" step at 32 rows, FP8 (E4M3) weights against bf16 from the same process, and
    the microseconds per token of a 24-layer engine both ways (logged like every other experiment of this file).  Same method as
    the rest of this file: warm, 24 layers' worth of distinct weights per shape, 4 passes per captured graph, 20 replays."""
    from indextts.utils import quant
    import weights as synth_weights
    from indextts.gpt.engine import GPTEngine
    log(f"==== w8 microbench {time.strftime('%H:%M:%S')} B={B} (us per launch, graph replay; bf16 | fp8 weights)")
    log(f"library: {os.path.basename(os.environ['ITTS_HIP_LIB'])}")
    R, V = 4, 8194
    hb = torch.randn(nat.packed_rows(B) * D, device=dev).to(T)
    fb = torch.randn(nat.packed_rows(B) * 4 * D, device=dev).to(T)
    ab = torch.randn(nat.packed_rows(B) * D, device=dev).to(T)
    hres = torch.randn(B, D, device=dev)
    q, lg = torch.zeros(B, D, device=dev, dtype=T), torch.zeros(B, V, device=dev)
    smax = 320
    kc = torch.zeros(L, B, H, smax, 64, device=dev, dtype=T)
    vc = torch.zeros(L, B, H, smax, 64, device=dev, dtype=T)
    pos = torch.full((1,), 150, dtype=torch.int32, device=dev)
    c3, c4 = torch.zeros(3 * D, device=dev), torch.zeros(4 * D, device=dev)     # ln_c of the folded forms

    def pair(K, N):
        w = torch.randn(K, N, device=dev) * 0.02
        codes, scale = quant.quantize_e4m3_cols(w)
        return nat.pack_weight(w.to(T)), nat.pack_weight_w8(codes), scale.contiguous()
    shapes = {
        "QKV' 1280x3840 fold + KV append": (D, 3 * D, lambda i: dict(x=hb, x_packed=True, epi=nat.EPI_QKV_CACHE, y=q, kcache=kc[i], vcache=vc[i],
                                                                     pos=pos, heads=H, smax=smax, ln_c=c3)),
        "out-proj 1280x1280 resid": (D, D, lambda i: dict(x=ab, x_packed=True, epi=nat.EPI_RESID_F32, yf=hres, y=hb, y_packed=True, rows_per_wg=16)),
        "FC' 1280x5120 fold + gelu": (D, 4 * D, lambda i: dict(x=hb, x_packed=True, epi=nat.EPI_GELU_STORE, y=fb, y_packed=True,
                                                               ln_c=c4)),
        "FC2 5120x1280 resid": (4 * D, D, lambda i: dict(x=fb, x_packed=True, epi=nat.EPI_RESID_F32, yf=hres, y=hb, y_packed=True, rows_per_wg=16)),
        "mel_head 1280x8194": (D, V, lambda i: dict(x=hb, x_packed=True, epi=nat.EPI_STORE_F32, yf=lg)),
    }
    for name, (K, N, kwf) in shapes.items():
        ws = [pair(K, N) for _ in range(L)]
        bias = torch.zeros(N, device=dev)
        kws = [kwf(i) for i in range(L)]

        def run16():
            for _ in range(R):
                for i in range(L):
                    nat.gemm_skinny(T, B, N, K, ws[i][0], bias, **kws[i])

        def run8():
            for _ in range(R):
                for i in range(L):
                    nat.gemm_skinny_w8(T, B, N, K, ws[i][1], ws[i][2], bias, **kws[i])
        u16, u8 = timed_graph(run16, R * L), timed_graph(run8, R * L)
        log(f"{name:34s} bf16 {u16:6.2f} us ({K * N * 2 / u16 / 1e6:5.2f} TB/s) | fp8 {u8:6.2f} us ({K * N / u8 / 1e6:5.2f} TB/s)")
        del ws
    Wsd = {k: v.float() for k, v in synth_weights.gpt_state_dict(L, with_conditioner=False).items()}
    emb = torch.randn(B, 60, D) * 0.5
    pad = torch.zeros(B, dtype=torch.int32)
    sp = dict(do_sample=True, top_p=0.8, top_k=30, temperature=1.0, repetition_penalty=10.0, seed=1)
    steps = 120
    for wd in (None, "fp8"):
        eng = GPTEngine(Wsd, L, D, H, dtype=T, device=dev, weight_dtype=wd)
        best = float("inf")
        for rep in range(3):      # the first run captures the graph and is not counted
            eng.prefill(emb, pad, steps + 2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode(steps, sp, force_stop=[steps - 1] * B, check_every=steps)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / (steps - 1) * 1e6
            best = min(best, dt) if rep > 0 else best
        log(f"engine 24 layers, {B} rows, weights {wd or 'bf16'}: {best:7.1f} us / token ({eng.weight_bytes / 1e6:.0f} MB streamed per token)")
        del eng
        torch.cuda.empty_cache()


def kv8_report():
    """--kv8: itts_attn_decode (paged, 16-bit pool; its QKV GEMM appends) against itts_attn_decode_kv8 (E4M3 pool; appends itself)
    per launch at config 3's contexts (75 / 151 / 216 keys), 32 rows, 24 layers' distinct pools; then the QKV GEMM with the
    KV-append epilogue against the row-major STORE epilogue the FP8 cache uses; then a 24-layer engine's us per token, 16-bit
    against FP8 cache, with bf16 and with FP8 weights.  Same method as the rest of this file."""
    import weights as synth_weights
    from indextts.gpt.engine import GPTEngine
    log(f"==== kv8 microbench {time.strftime('%H:%M:%S')} B={B} (us per launch, graph replay; 16-bit | fp8 KV cache)")
    log(f"library: {os.path.basename(os.environ['ITTS_HIP_LIB'])}")
    R, bs = 4, 16
    nblk = 320 // bs
    tab = torch.zeros(B, 64, dtype=torch.int32)
    tab[:, :nblk] = (1 + torch.randperm(B * nblk)).view(B, nblk).to(torch.int32)
    tab = tab.to(dev)
    blocks = 1 + B * nblk
    kc16 = torch.randn(L, blocks, H, bs, 64, device=dev).to(T)
    vc16 = torch.randn(L, blocks, H, bs, 64, device=dev).to(T)
    kc8 = (torch.randn(L, blocks, H, bs, 64, device=dev) * 16).to(torch.float8_e4m3fn).view(torch.uint8)
    vc8 = (torch.randn(L, blocks, H, bs, 64, device=dev) * 16).to(torch.float8_e4m3fn).view(torch.uint8)
    scale = torch.full((L, 2, H), 2.0 ** -4, device=dev)
    q = torch.randn(B, D, device=dev).to(T)
    qkv = torch.randn(B, 3 * D, device=dev).to(T)
    a = torch.zeros(nat.packed_rows(B) * D, device=dev, dtype=T)
    pad = torch.zeros(B, dtype=torch.int32, device=dev)
    for ctx in (75, 151, 216):
        pos = torch.full((1,), ctx - 1, dtype=torch.int32, device=dev)

        def run16():
            for _ in range(R):
                for i in range(L):
                    nat.attn_decode(q, kc16[i], vc16[i], a, pad, pos, B, H, 0, out_packed=True, kv_tab=tab, kv_bs=bs)

        def run8():
            for _ in range(R):
                for i in range(L):
                    nat.attn_decode_kv8(qkv, kc8[i], vc8[i], a, pad, pos, scale[i], B, H, out_packed=True, kv_tab=tab, kv_bs=bs)
        u16, u8 = timed_graph(run16, R * L), timed_graph(run8, R * L)
        by = B * ctx * 2 * D
        log(f"attn_decode ctx={ctx:3d}  16-bit {u16:6.2f} us ({by * 2 / u16 / 1e6:5.2f} TB/s) | fp8 + append {u8:6.2f} us ({by / u8 / 1e6:5.2f} TB/s)")
    hb = torch.randn(nat.packed_rows(B) * D, device=dev).to(T)
    c3, b3 = torch.zeros(3 * D, device=dev), torch.zeros(3 * D, device=dev)
    ws = [rand_w(D, 3 * D) for _ in range(L)]
    pos = torch.full((1,), 150, dtype=torch.int32, device=dev)

    def qkv_cache():
        for _ in range(R):
            for i in range(L):
                nat.gemm_skinny(T, B, 3 * D, D, ws[i], b3, x=hb, x_packed=True, epi=nat.EPI_QKV_CACHE, y=q, kcache=kc16[i], vcache=vc16[i],
                                pos=pos, heads=H, smax=0, ln_c=c3, kv_tab=tab, kv_bs=bs)

    def qkv_store():
        for _ in range(R):
            for i in range(L):
                nat.gemm_skinny(T, B, 3 * D, D, ws[i], b3, x=hb, x_packed=True, epi=nat.EPI_STORE, y=qkv, ln_c=c3)
    log(f"QKV' 1280x3840 fold: KV-append epilogue {timed_graph(qkv_cache, R * L):6.2f} us | row-major STORE {timed_graph(qkv_store, R * L):6.2f} us")
    del ws, kc16, vc16, kc8, vc8
    torch.cuda.empty_cache()
    Wsd = {k: v.float() for k, v in synth_weights.gpt_state_dict(L, with_conditioner=False).items()}
    emb = torch.randn(B, 60, D) * 0.5
    pad_h = torch.zeros(B, dtype=torch.int32)
    sp = dict(do_sample=True, top_p=0.8, top_k=30, temperature=1.0, repetition_penalty=10.0, seed=1)
    steps = 120
    for wd in (None, "fp8"):
        for kvd in (None, "fp8"):
            eng = GPTEngine(Wsd, L, D, H, dtype=T, device=dev, weight_dtype=wd, kv_dtype=kvd)
            if kvd:
                eng.calibrate_kv_scales(emb, pad_h)
            best, pre = float("inf"), float("inf")
            for rep in range(3):      # the first run captures the graph and is not counted
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.prefill(emb, pad_h, steps + 2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.decode(steps, sp, force_stop=[steps - 1] * B, check_every=steps)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) / (steps - 1) * 1e6
                if rep > 0:
                    best, pre = min(best, dt), min(pre, (t1 - t0) * 1e3)
            pool = (eng.kv.kc.numel() * eng.kv.kc.element_size() * 2) / 1e6
            log(f"engine 24 layers, {B} rows, weights {wd or 'bf16'}, KV cache {kvd or '16-bit'}: {best:7.1f} us / token, prefill {pre:6.2f} ms, "
                f"pool {pool:.1f} MB, {eng.step_bytes(B, 151) / 1e6:.0f} MB per token at 151 keys")
            del eng
            torch.cuda.empty_cache()


if "--kv8" in sys.argv[1:]:
    kv8_report()
    sys.exit(0)

if "--w8" in sys.argv[1:]:
    w8_report()
    sys.exit(0)

log(f"==== microbench {time.strftime('%H:%M:%S')} B={B}")
tokens = torch.zeros(B, dtype=torch.int32, device=dev)
state = torch.zeros(8, dtype=torch.int32, device=dev)
state[1] = 150
table = torch.randn(8194, D, device=dev)
ptab = torch.randn(803, D, device=dev)
h = torch.randn(B, D, device=dev)
xn = torch.randn(B, D, device=dev).to(T)
f = torch.randn(B, 4 * D, device=dev).to(T)
q = torch.randn(B, D, device=dev).to(T)
a = torch.randn(B, D, device=dev).to(T)
slab = torch.randn(4, B, D, device=dev)
lw, lb = torch.ones(D, device=dev), torch.zeros(D, device=dev)
bias_d = torch.zeros(D, device=dev)
bias_3d = torch.zeros(3 * D, device=dev)
bias_4d = torch.zeros(4 * D, device=dev)
smax = 320
kc = torch.randn(L, B, H, smax, 64, device=dev).to(T)
vc = torch.randn(L, B, H, smax, 64, device=dev).to(T)
pad = torch.zeros(B, dtype=torch.int32, device=dev)
pos = state[1:2]
w_qkv = [rand_w(D, 3 * D) for _ in range(L)]
w_o = [rand_w(D, D) for _ in range(L)]
w_fc = [rand_w(D, 4 * D) for _ in range(L)]
w_pr = [rand_w(4 * D, D) for _ in range(L)]

R = 4  # passes over the 24 layers per graph


def exp_embed():
    for _ in range(R * L):
        nat.embed_step(tokens, table, ptab, state[0:1], 1, h)


def exp_ln0():
    for _ in range(R * L):
        nat.ln_reduce(h, lw, lb, xn)


def exp_ln4():
    for _ in range(R * L):
        nat.ln_reduce(h, lw, lb, xn, slab=slab, nslab=4, bias=bias_d)


def exp_qkv():
    for _ in range(R):
        for i in range(L):
            nat.gemm_skinny(T, B, 3 * D, D, w_qkv[i], bias_3d, x=xn, epi=nat.EPI_QKV_CACHE, y=q, kcache=kc[i], vcache=vc[i],
                            pos=pos, heads=H, smax=smax)


def exp_attn():
    for _ in range(R):
        for i in range(L):
            nat.attn_decode(q, kc[i], vc[i], a, pad, pos, B, H, smax)


def exp_proj(ks):
    def fn():
        for _ in range(R):
            for i in range(L):
                nat.gemm_skinny(T, B, D, D, w_o[i], None, x=a, epi=nat.EPI_SLAB_F32, yf=slab, ksplit=ks)
    return fn


def exp_fc():
    for _ in range(R):
        for i in range(L):
            nat.gemm_skinny(T, B, 4 * D, D, w_fc[i], bias_4d, x=xn, epi=nat.EPI_GELU_STORE, y=f)


def exp_fc2(ks):
    def fn():
        for _ in range(R):
            for i in range(L):
                nat.gemm_skinny(T, B, D, 4 * D, w_pr[i], None, x=f, epi=nat.EPI_SLAB_F32, yf=slab, ksplit=ks)
    return fn


MB = 1e-6
for name, fn, bytes_ in [
    ("embed_step (trivial floor)", exp_embed, 0),
    ("ln_reduce nslab=0", exp_ln0, 0),
    ("ln_reduce nslab=4", exp_ln4, 0),
    ("skinny QKV 1280x3840", exp_qkv, D * 3 * D * 2),
    ("attn_decode ctx=151", exp_attn, B * 151 * 2 * D * 2),
    ("skinny proj ksplit=4", exp_proj(4), D * D * 2),
    ("skinny proj ksplit=2", exp_proj(2), D * D * 2),
    ("skinny FC 1280x5120", exp_fc, D * 4 * D * 2),
    ("skinny FC2 ksplit=4", exp_fc2(4), D * 4 * D * 2),
    ("skinny FC2 ksplit=2", exp_fc2(2), D * 4 * D * 2),
]:
    us = timed_graph(fn, R * L)
    extra = f"  {bytes_ * MB:6.1f} MB -> {bytes_ / us / 1e6:6.2f} TB/s" if bytes_ else ""
    log(f"{name:32s} {us:7.2f} us/launch{extra}")

# ---- balance experiment: column tiles vs the 256 CUs
for N in (3840, 4096, 4112, 5120, 6144, 8192):
    ws = [rand_w(D, N) for _ in range(L)]
    yb = torch.zeros(B, N, device=dev, dtype=T)
    bb = torch.zeros(N, device=dev)

    def fn():
        for _ in range(R):
            for i in range(L):
                nat.gemm_skinny(T, B, N, D, ws[i], bb, x=xn, epi=nat.EPI_GELU_STORE, y=yb)
    us = timed_graph(fn, R * L)
    log(f"skinny K=1280 N={N:5d} ({N // 16:3d} tiles) {us:7.2f} us  {D * N * 2 / us / 1e6:5.2f} TB/s")
    del ws

# ---- sweep (ksplit, tiles per workgroup, waves) for the two N=1280 GEMMs and FC
slab8 = torch.randn(8, B, D, device=dev)
for name, K, ws, xin in (("proj", D, w_o, a), ("FC2", 4 * D, w_pr, f)):
    for ks in (2, 3, 4, 6, 8):
        for ntb in (1, 2):
            def fn(ks=ks, ws=ws, xin=xin, K=K):
                for _ in range(R):
                    for i in range(L):
                        nat.gemm_skinny(T, B, D, K, ws[i], None, x=xin, epi=nat.EPI_SLAB_F32, yf=slab8, ksplit=ks)
            nat.debug_set(1, ntb)
            us = timed_graph(fn, R * L)
            log(f"{name} ksplit={ks} ntb={ntb}: {us:6.2f} us  (blocks {((80 + ntb - 1) // ntb) * ks})")
nat.debug_set(1, 0)
for ntb in (1, 2, 3):
    for nw in (4, 8):
        nat.debug_set(1, ntb)
        nat.debug_set(2, nw)
        us = timed_graph(exp_fc, R * L)
        log(f"FC ntb={ntb} nw={nw}: {us:6.2f} us")
nat.debug_set(1, 0)
nat.debug_set(2, 0)
for ns in (3, 6, 8):
    def fn(ns=ns):
        for _ in range(R * L):
            nat.ln_reduce(h, lw, lb, xn, slab=slab8, nslab=ns, bias=bias_d)
    log(f"ln_reduce nslab={ns}: {timed_graph(fn, R * L):6.2f} us")
