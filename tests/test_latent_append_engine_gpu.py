"""GPTEngine.latent_cache / latent_append on the GPU: the incremental latent pass in chunks against latent() over the whole
sequences, on the 2-layer full-width synthetic model, two rows of different prompt lengths in one call (cache rows in
non-identity order), for every engine kind.

fp32: BIT-EQUAL.  _proj_ksplit is 1 in fp32, the plain GEMM's K loop does not depend on M, LayerNorm is per row and the append
attention keeps the packed form's key tiling (tests/test_latent_append_kernels_gpu.py).
16-bit (bf16 / fp16 activations; the bank, the FP8 KV cache and FP8 weights under bf16): _proj_ksplit(M) changes the split-K
factor with the row count, so the two paths differ in summation order.  Both are compared with the fp32 engine's latents on the
same sequences (same voices): the incremental path holds the 16-bit bound of the existing latent checks (RMS
< 1e-2 on latents of RMS ~ 1), and its max-abs error stays within twice the whole pass's -- both are 16-bit roundings of the
same fp32 computation that differ only in where partial sums are rounded, errors of one distribution; the measured figures are
in profiles/stream_latent_cache.txt (`-s` prints them).  The fp8-WEIGHT engine computes with other (quantised) weights than the
fp32 engine, a difference tests/test_w8_engine_gpu.py pins against the oracle on the dequantised weights; here its incremental
pass is held to the same RMS bound against its OWN whole pass, and the distance of both to the fp32 engine is printed."""
import numpy as np
import pytest
import torch

import weights
from refill_voices import make_factors

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPT, MEL = [45, 30], 64                 # rows of cond | text per element; start | codes rows behind them
CHUNKS = (7, 16, 1, 40)                    # the first call carries prompt + 7 rows
ROWS = [1, 0]                              # element b lives in cache row ROWS[b]
KINDS = {
    "fp32": dict(gpt="fp32"), "fp32-ids": dict(gpt="fp32", voices=dict(adapter_ids=[1, 2])),
    "fp32-mix": dict(gpt="fp32", voices=dict(adapter_mix=[{0: 0.5, 2: 0.25}, 1])),
    "bf16": dict(gpt="bf16"), "fp16": dict(gpt="fp16"), "bf16-ids": dict(gpt="bf16", voices=dict(adapter_ids=[1, 2])),
    "bf16-mix": dict(gpt="bf16", voices=dict(adapter_mix=[{0: 0.5, 2: 0.25}, 1])),
    "bf16-kv8": dict(gpt="bf16", kv_cache="fp8"), "w8": dict(gpt="fp8"),
}


@pytest.fixture(scope="module")
def state():
    return weights.gpt_state_dict(2), weights.bigvgan_state_dict()


@pytest.fixture(scope="module")
def engines(state):
    made = {}

    def get(gpt="fp32", bank=False, **prec):
        key = (gpt, bank, tuple(sorted(prec.items())))
        if key not in made:
            from indextts.infer import IndexTTS
            cfg = weights.reference_config()
            cfg["gpt"]["layers"] = 2
            tts = IndexTTS.from_weights(cfg, state[0], state[1], device="cuda:0", precision_config=dict(gpt=gpt, vocoder="fp32", **prec))
            if bank:
                tts.gpt.attach_lora_bank(make_factors(state[0], (4, 8, 16), (2.0, 1.0, 0.5)))
            made[key] = tts
        return made[key].gpt.engine
    return get


@pytest.fixture(scope="module")
def emb():
    """[2, S, D] fp32 rows of unit scale (any rows are a sequence to latent()), right-padded with zeros"""
    g = torch.Generator().manual_seed(77)
    tot = [p + MEL for p in PROMPT]
    e = torch.zeros(2, max(tot), 1280)
    for b, n in enumerate(tot):
        e[b, :n] = torch.randn(n, 1280, generator=g) * 0.5
    return e.to(DEV), tot


def whole_pass(eng, emb, tot, voices):
    out = eng.latent(emb, lengths=tot, **voices)
    return [out[b, PROMPT[b]: tot[b]].clone() for b in range(2)]


def chunked(eng, emb, tot, voices, rows=ROWS):
    cache = eng.latent_cache(2, max(tot))
    assert cache.cap == 128 and cache.kc.shape == (2, 2, 20, 128, 64) and not cache.have.any()
    got, at = [[], []], [0, 0]
    for i, c in enumerate(CHUNKS):
        n = [(PROMPT[b] if i == 0 else 0) + c for b in range(2)]
        part = torch.cat([emb[b, at[b]: at[b] + n[b]] for b in range(2)])
        keep = part.clone()
        out = eng.latent_append(cache, part, n, rows, **voices)
        assert torch.equal(part, keep)                      # the caller's rows are not the pass's scratch
        o = 0
        for b in range(2):
            got[b].append(out[o + (PROMPT[b] if i == 0 else 0): o + n[b]])
            o, at[b] = o + n[b], at[b] + n[b]
        assert [int(cache.have[r]) for r in rows] == at
    return [torch.cat(g) for g in got], cache


@pytest.mark.parametrize("kind", list(KINDS))
def test_chunks_against_the_whole_pass(engines, emb, kind):
    spec = dict(KINDS[kind])
    voices = spec.pop("voices", {})
    e, tot = emb
    eng = engines(bank=bool(voices), **spec)
    inc, cache = chunked(eng, e, tot, voices)
    whole = whole_pass(eng, e, tot, voices)
    if spec["gpt"] == "fp32":
        for b in range(2):
            assert torch.equal(inc[b], whole[b]), f"{kind}: row {b} max-abs {(inc[b] - whole[b]).abs().max().item():.3e}"
        return
    ref = whole_pass(engines(bank=bool(voices)), e, tot, voices)
    for b in range(2):
        scale = ref[b].pow(2).mean().sqrt().item()
        e_inc, e_whole = (inc[b] - ref[b]).abs().max().item(), (whole[b] - ref[b]).abs().max().item()
        rms_inc, rms_whole = (inc[b] - ref[b]).pow(2).mean().sqrt().item(), (whole[b] - ref[b]).pow(2).mean().sqrt().item()
        rms_own = (inc[b] - whole[b]).pow(2).mean().sqrt().item()
        print(f"latent_append parity | {kind} | row {b} | latent rms = {scale:.3f} | against fp32: incremental max-abs = {e_inc:.3e} rms = "
              f"{rms_inc:.3e}; whole max-abs = {e_whole:.3e} rms = {rms_whole:.3e} | incremental against whole rms = {rms_own:.3e}")
        if kind == "w8":
            assert rms_own < 1e-2, rms_own
        else:
            assert rms_inc < 1e-2, rms_inc
            assert e_inc <= 2 * e_whole, (e_inc, e_whole)


def test_refusals_and_reset(engines, emb):
    e, tot = emb
    eng = engines()
    with pytest.raises(ValueError, match="budget"):
        eng.latent_cache(4096, 4096)
    _, cache = chunked(eng, e, tot, {})
    row = e[0, :4].contiguous()
    with pytest.raises(ValueError, match="twice"):
        eng.latent_append(cache, torch.cat([row, row]), [4, 4], [0, 0])
    with pytest.raises(ValueError, match="do not fit"):
        eng.latent_append(cache, e[0, :100].contiguous(), [100], [0])
    banked = engines(bank=True)
    c2 = banked.latent_cache(1, 64)
    banked.latent_append(c2, row, [4], [0], adapter_ids=[1])
    with pytest.raises(ValueError, match="another voice"):
        banked.latent_append(c2, row, [4], [0], adapter_ids=[2])
    c2.reset(0)
    banked.latent_append(c2, row, [4], [0], adapter_ids=[2])
    assert int(c2.have[0]) == 4
    # a reset row starts over: the same rows give the same bits although the old positions were never cleared
    cache.reset(1)
    first = eng.latent_append(cache, e[0, :50].contiguous(), [50], [1])
    assert torch.equal(first[PROMPT[0]:], whole_pass(eng, e, tot, {})[0][: 50 - PROMPT[0]])


def test_interleaved_appends_disturb_nothing(engines, state):
    """latent_append after EVERY burst of decode_chunks: the loop's later tokens are those of the uninterrupted loop (the shape of
    tests/test_stream_gpu.py::test_interleaved_passes_disturb_nothing)."""
    import synth
    from indextts.gpt.model import sampling_params
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    tts = IndexTTS.from_weights(cfg, state[0], state[1], device="cuda:0", precision_config=dict(gpt="bf16", vocoder="fp32"))
    eng = tts.gpt.engine
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    text = torch.from_numpy(np.random.default_rng(11).integers(2, 12000, size=12)).to(torch.int32)
    g, _ = tts._gen_kwargs(dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1))
    sp = sampling_params(g, 9)
    conds, _ = tts._prompt_features(cond_mel)

    def prefill():
        emb, pad = tts.gpt.prefix_rows(conds, text[None])
        eng.prefill(emb, pad, 48, shared_rows=int(conds.shape[1]))
    prefill()
    want = eng.decode(48, dict(sp), force_stop=[40]).cpu()
    prefill()
    from indextts.infer import _LatentRows
    lc, ran = _LatentRows(eng, 1, 256), 0
    for codes, fin in eng.decode_chunks(48, dict(sp), 8, force_stop=[40]):
        n = codes.shape[1]
        assert torch.equal(codes, want[:, :n]), n
        if not bool(fin[0]):
            lat = tts._latents_incremental(lc, [0], conds, [text], [codes[0]])[0]
            assert lat.shape[0] == n and bool(torch.isfinite(lat).all())
            ran += 1
    assert ran == 5 and torch.equal(codes, want) and lc.fed[0] == 40
