"""Host-side structure of the decode engine, without a GPU: the native launches are replaced by recorders.
  * gemm_launches_of_step (bench.py's roofline, tools/pmc_decode_gemm.py) traces the skinny GEMMs of the real decode step;
  * the key of a captured decode step changes with every setting the captured launches read;
  * decode_refill's admission never over-commits the paged block pool."""
from types import SimpleNamespace

import pytest
import torch

from indextts import _native as nat
from indextts.gpt.engine import GPTEngine, PagedKV, admit

torch.set_grad_enabled(False)
L, H, V = 2, 2, 40
D = 64 * H


def tiny_weights():
    g = torch.Generator().manual_seed(5)
    shapes = {"gpt.ln_f.weight": (D,), "gpt.ln_f.bias": (D,), "final_norm.weight": (D,), "final_norm.bias": (D,),
              "mel_head.weight": (V, D), "mel_head.bias": (V,), "mel_embedding.weight": (V, D),
              "mel_pos_embedding.emb.weight": (64, D), "text_embedding.weight": (V, D), "text_pos_embedding.emb.weight": (64, D)}
    for i in range(L):
        p = f"gpt.h.{i}."
        shapes.update({p + "ln_1.weight": (D,), p + "ln_1.bias": (D,), p + "attn.c_attn.weight": (D, 3 * D),
                       p + "attn.c_attn.bias": (3 * D,), p + "attn.c_proj.weight": (D, D), p + "attn.c_proj.bias": (D,),
                       p + "ln_2.weight": (D,), p + "ln_2.bias": (D,), p + "mlp.c_fc.weight": (D, 4 * D),
                       p + "mlp.c_fc.bias": (4 * D,), p + "mlp.c_proj.weight": (4 * D, D), p + "mlp.c_proj.bias": (D,)})
    return {k: torch.randn(s, generator=g) * 0.02 for k, s in shapes.items()}


def _arg(v):
    return ("tensor", v.data_ptr(), tuple(v.shape), v.dtype) if torch.is_tensor(v) else v


@pytest.fixture
def recorded(monkeypatch):
    """A CPU engine whose native calls are recorded: calls["gemm_skinny"] lists every skinny GEMM with its arguments."""
    calls = {"gemm_skinny": [], "other": 0}

    def gemm(*a, **kw):
        calls["gemm_skinny"].append((tuple(_arg(v) for v in a), tuple(sorted((k, _arg(v)) for k, v in kw.items()))))

    def other(*a, **kw):
        calls["other"] += 1
    monkeypatch.setattr(nat, "pack_weight", lambda w: w.contiguous())
    monkeypatch.setattr(nat, "pack_weight_w8", lambda codes: codes.contiguous())
    monkeypatch.setattr(nat, "gemm_skinny", gemm)
    for name in ("embed_step", "attn_decode", "attn_decode_kv8", "ln_reduce"):
        monkeypatch.setattr(nat, name, other)

    def make(mode, B, lora=False, paged=False, **kw):
        monkeypatch.setenv("ITTS_DECODE_MODE", mode)
        eng = GPTEngine(tiny_weights(), L, D, H, dtype=torch.bfloat16, device="cpu", **kw)
        if lora:
            r = 8
            ad = {f"gpt.h.{i}.{n}": (torch.randn(r, k) * 0.1, torch.randn(D, r) * 0.1)
                  for i in range(L) for n, k in (("attn.c_proj", D), ("mlp.c_proj", 4 * D))}
            eng.attach_lora(ad, 2.0)
        eng._ensure(B, 64, paged=paged, blocks=16)
        return eng
    return make, calls


def _gemms_of(calls, fn):
    calls["gemm_skinny"].clear()
    calls["other"] = 0
    out = fn()
    return list(calls["gemm_skinny"]), calls["other"], out


@pytest.mark.parametrize("mode", ["fold", "launch"])
@pytest.mark.parametrize("B", [32, 96])
@pytest.mark.parametrize("lora", [False, True])
def test_gemm_launches_of_step_are_the_decode_steps_gemms(recorded, mode, B, lora):
    make, calls = recorded
    eng = make(mode, B, lora)
    state = eng.state.clone()
    traced, others, (n, nbytes) = _gemms_of(calls, lambda: eng.gemm_launches_of_step(B))
    assert others == 0 and n == len(traced) == 4 * L + 1
    assert not getattr(eng, "_pending_bump", False) and torch.equal(eng.state, state)   # the loop state is left alone
    real, others, _ = _gemms_of(calls, lambda: eng._step_transformer(B))
    assert others > 0 and traced == real
    if lora:   # the out-projections carry the adapter's extra columns: N = D + 16
        assert sorted({c[0][2] for c in real}) == sorted({3 * D, 4 * D, D + 16, V})
    if B == 32 and not lora:
        es, KS = 2, eng.KSPLIT   # the closed form bench.py's algorithmic_MB_per_launch was computed with
        per_layer = 12 * D * D * es + B * D * es * (1 + 1 + 1 + 4) + B * es * (3 * D + 4 * D)
        per_layer += 2 * (2 * B * D * 4 + B * D * es) if mode == "fold" else 2 * KS * B * D * 4
        assert nbytes == L * per_layer + V * D * es + B * D * es + B * V * 4
        assert nbytes == {"fold": 1203200, "launch": 1235968}[mode]


@pytest.mark.parametrize("B", [32, 96])
@pytest.mark.parametrize("weight_dtype, kv_dtype", [("fp8", None), (None, "fp8"), ("fp8", "fp8")])
def test_gemm_launches_of_the_fp8_steps(recorded, B, weight_dtype, kv_dtype):
    """The folded step over FP8 weights, an FP8 KV cache and both: the same five launches per block, the weight scales ride on the
    four GEMMs (and the head) of an FP8-weight engine and on none of a 16-bit one, one byte per weight in the tally."""
    make, calls = recorded
    eng = make("fold", B, paged=kv_dtype is not None, weight_dtype=weight_dtype, kv_dtype=kv_dtype)
    traced, others, (n, nbytes) = _gemms_of(calls, lambda: eng.gemm_launches_of_step(B))
    assert others == 0 and n == len(traced) == 4 * L + 1
    real, others, _ = _gemms_of(calls, lambda: eng._step_transformer(B))
    assert others == L + 2 and traced == real              # embed, one attention per block, the final norms: nothing else
    scaled = [dict(kw).get("w_scale") is not None for _, kw in real]
    assert scaled == [weight_dtype == "fp8"] * len(real)
    epis = [dict(kw)["epi"] for _, kw in real[:4]]
    assert epis == [nat.EPI_STORE if kv_dtype else nat.EPI_QKV_CACHE, nat.EPI_RESID_F32, nat.EPI_GELU_STORE, nat.EPI_RESID_F32]
    if B == 32:
        es, ws = 2, 1 if weight_dtype else 2
        per_layer = 12 * D * D * ws + B * D * es * (1 + 1 + 1 + 4) + B * es * (3 * D + 4 * D) + 2 * (2 * B * D * 4 + B * D * es)
        assert nbytes == L * per_layer + V * D * ws + B * D * es + B * V * 4


def test_graph_key_covers_every_setting_of_the_captured_step(recorded):
    make, _ = recorded
    eng = make("fold", 32)
    sp = dict(do_sample=True, top_p=0.8, top_k=30, temperature=1.0, repetition_penalty=10.0, seed=0)
    base = eng._graph_key("token", 32, sp)
    changes = dict(decode_mode="launch", lora=True, fold_rows=[32, 16], fold_rows_consumers=16, fold_wide=True, pa=False,
                   KSPLIT=6, skip_finished=False, share_kv_reads=False, beam_kv="copy", kv=SimpleNamespace(bs=32))
    for attr, value in changes.items():
        old = getattr(eng, attr)
        setattr(eng, attr, value)
        assert eng._graph_key("token", 32, sp) != base, attr
        setattr(eng, attr, old)
    assert eng._graph_key("token", 32, sp) == base
    assert eng._graph_key("beam", 32, sp) != base and eng._graph_key("token", 33, sp) != base
    assert eng._graph_key("token", 32, sp, nb=3) != base and eng._graph_key("token", 32, dict(sp, top_k=31)) != base
    assert eng._graph_key("token", 32, dict(reversed(list(sp.items())))) == base


def _prefilled_pool(pads, S, max_new_prefill, bs=16):
    """A PagedKV sized and dealt the way plain prefill(max_new_prefill) does it (no slots_window)."""
    span = lambda lo, hi: ((hi - 1) // bs) - (lo // bs) + 1   # noqa: E731
    need = sum(span(p, S + max_new_prefill + 1) for p in pads)
    kv = PagedKV(1, 1, len(pads), need + 1, bs, torch.float32, "cpu")
    for b, p in enumerate(pads):
        kv.cover(b, p, S + max_new_prefill + 1)
    return kv


def _items(*lengths):
    return [(torch.zeros(n, 1), -1) for n in lengths]


def test_admission_hands_back_what_no_longer_fits():
    S, max_new, ce = 40, 40, 4
    kv = _prefilled_pool([0, 5, 10], S, max_new + ce + 1)
    assert not kv.free
    for b, p in enumerate([0, 5, 10]):           # decode_refill's extension of the prefilled rows needs no new block
        kv.cover(b, p, S + max_new + ce)
    assert not kv.free
    kv.release(0)
    kv.release(1)
    free = len(kv.free)
    # two slots free: the first item's window takes 7 blocks, the second no longer fits the 5 left -- handed back, not raised
    end = 110
    assert kv.blocks_of(end - 51, end + max_new + ce) == 7 and free == 12
    assert admit(kv, [0, 1], _items(50, 50), end, max_new, ce) == 1
    assert len(kv.free) == free - 7 and kv.span[1] is None
    # a prompt whose own window exceeds the block table's is handed back whatever the pool holds
    kv.release(0)
    kv.release(2)
    assert admit(kv, [0, 2], _items(kv.window, 3), 2000, max_new, ce) == 0
    assert admit(kv, [0, 2], _items(3, 3), 2000, max_new, ce) == 2


def test_staggered_admissions_never_overcommit_the_pool():
    """The refill loop's block traffic on a pool from plain prefill(max_new + ce + 1): rows stop at staggered steps, their
    blocks go back, new rows are admitted with their whole windows at once; nothing ever raises and the pool is never
    exceeded -- what does not fit waits as leftover."""
    S, max_new, ce, slots = 40, 40, 4, 4
    pads = [0, 3, 6, 9]
    kv = _prefilled_pool(pads, S, max_new + ce + 1)
    for b, p in enumerate(pads):
        kv.cover(b, p, S + max_new + ce)
    queue = [20, 37, 12, 39, 30, 25, 38, 15, 36, 33, 18, 39]
    ends = {b: S + 10 * (b + 1) for b in range(slots)}    # the step (as a position) at which each row stops
    placed, leftover = 0, []
    for n in range(ce + 1, 2000, ce):
        end = S + n + ce - 1                              # staged: the new rows join at the next poll
        free = [b for b in range(slots) if b in ends and ends[b] <= S + n]
        for b in free:
            kv.release(b)
            del ends[b]
        free = [b for b in range(slots) if b not in ends]
        if free and queue and not leftover:
            items = _items(*queue[: len(free)])
            queue = queue[len(items):]
            k = admit(kv, free, items, end, max_new, ce)
            leftover = items[k:]
            for j, b in enumerate(free[:k]):
                ends[b] = end + 7 * (placed + j) % max_new
            placed += k
            assert kv.used_blocks() <= kv.blocks - 1
        if not ends:
            break
    assert placed + len(leftover) + len(queue) == 12 and placed > 0
    assert kv.used_blocks() == 0
