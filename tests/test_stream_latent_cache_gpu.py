"""latent_cache=True of stream_utterance / stream_batch / stream_queue / infer_stream / /tts/stream on the GPU (the incremental
latent pass, GPTEngine.latent_append) against latent_cache=False and the whole-utterance paths, on the 2-layer full-width
synthetic model of tests/test_stream_gpu.py.

Rules.  The codes never depend on the latent pass: identical.  fp32: tests/test_latent_append_engine_gpu.py establishes that the
incremental pass gives the bits of the whole pass, and the vocoder windows are cut alike, so the PCM has the BITS of
latent_cache=False.  bf16 GPT / fp16 vocoder: the existing bound of the streamed-against-whole comparison, 2 * 5e-3 = 1e-2 RMS in
[-1, 1] units against infer_batch / infer_queue (tests/test_stream_gpu.py, tests/test_stream_queue_gpu.py)."""
import warnings

import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMPLE = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1)
GREEDY = dict(do_sample=False, repetition_penalty=10.0, num_beams=1)
CHUNK, RMS_16BIT = 8, 2 * 5e-3


@pytest.fixture(scope="module")
def state():
    return weights.gpt_state_dict(2), weights.bigvgan_state_dict()


def make_tts(state, gpt="fp32", vocoder="fp32", **prec):
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    return IndexTTS.from_weights(cfg, state[0], state[1], device="cuda:0", precision_config=dict(gpt=gpt, vocoder=vocoder, **prec))


@pytest.fixture(scope="module")
def tts32(state):
    return make_tts(state)


@pytest.fixture(scope="module")
def tts16(state):
    return make_tts(state, "bf16", "fp16")


@pytest.fixture(scope="module")
def cond_mel():
    return torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(11)
    return [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (12, 5, 17, 9, 14)]


def rel_rms(got, want):
    return ((got - want) / 32767.0).pow(2).mean().sqrt().item()


def same_events(a, b):
    assert [(u, int(p.numel()), last) for u, p, last in a] == [(u, int(p.numel()), last) for u, p, last in b]
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- one utterance
def utterance(tts, cond_mel, text, T, **kw):
    trace = {}
    chunks = list(tts.stream_utterance(cond_mel, text, chunk_tokens=CHUNK, max_mel_tokens=T + 2 * CHUNK, seed=5, force_stop=[T],
                                       _trace=trace, **kw, **SAMPLE))
    return chunks, trace


def test_one_utterance_fp32_has_the_bits_of_the_repeated_pass(tts32, cond_mel, texts):
    off, t0 = utterance(tts32, cond_mel, texts[0], 88)
    on, t1 = utterance(tts32, cond_mel, texts[0], 88, latent_cache=True)
    assert torch.equal(t0["codes"], t1["codes"]) and t0["frames"] == t1["frames"] and len(on) == len(off) > 3
    assert all(torch.equal(a, b) for a, b in zip(t0["latent"], t1["latent"]))
    assert all(torch.equal(a, b) for a, b in zip(on, off))


@pytest.mark.parametrize("kind", ["bf16", "bf16-kv8"])
def test_one_utterance_16bit_holds_the_stream_bound(state, tts16, cond_mel, texts, kind):
    tts = tts16 if kind == "bf16" else make_tts(state, "bf16", "fp16", kv_cache="fp8")
    wavs, rows = tts.infer_batch(cond_mel, [texts[0]], max_mel_tokens=88 + 2 * CHUNK, force_stop=[88], seed=5, return_codes=True, **SAMPLE)
    on, trace = utterance(tts, cond_mel, texts[0], 88, latent_cache=True)
    assert torch.equal(trace["codes"], rows[0].long().cpu())
    got = torch.cat(on)
    assert got.shape == wavs[0].shape
    rms = rel_rms(got, wavs[0])
    print(f"stream latent cache | {kind} | one utterance, 88 frames, chunks of {CHUNK} | waveform rms against infer_batch = {rms:.3e}")
    assert rms <= RMS_16BIT, rms


# ---------------------------------------------------------------------------------------------------------------- a batch
ENDS3 = [44, 75, 60]


def batch_events(tts, cond_mel, rows, **kw):
    trace = {}
    ev = list(tts.stream_batch(cond_mel, rows, chunk_tokens=CHUNK, max_mel_tokens=96, seed=7, force_stop=ENDS3, _trace=trace, **kw, **GREEDY))
    return ev, trace


def test_a_batch_of_three_fp32_has_the_bits_of_the_repeated_pass(tts32, cond_mel, texts):
    off, t0 = batch_events(tts32, cond_mel, texts[:3])
    on, t1 = batch_events(tts32, cond_mel, texts[:3], latent_cache=True)
    assert all(torch.equal(a, b) for a, b in zip(t0["codes"], t1["codes"])) and t0["frames"] == t1["frames"]
    same_events(on, off)


def test_a_batch_of_three_16bit_holds_the_stream_bound(tts16, cond_mel, texts):
    wavs, rows = tts16.infer_batch(cond_mel, texts[:3], max_mel_tokens=96, force_stop=ENDS3, seed=7, return_codes=True, **GREEDY)
    on, trace = batch_events(tts16, cond_mel, texts[:3], latent_cache=True)
    for b in range(3):
        assert torch.equal(trace["codes"][b], rows[b].long().cpu())
        got = torch.cat([p for u, p, _ in on if u == b])
        rms = rel_rms(got, wavs[b])
        print(f"stream latent cache | bf16 | batch row {b}, {ENDS3[b]} frames | waveform rms against infer_batch = {rms:.3e}")
        assert got.shape == wavs[b].shape and rms <= RMS_16BIT, rms


# ---------------------------------------------------------------------------------------------------------------- the queue
ENDS5 = [44, 60, 38, 75, 52]


def queue_events(tts, cond_mel, rows, **kw):
    trace = {}
    ev = list(tts.stream_queue(cond_mel, rows, slots=2, chunk_tokens=CHUNK, max_mel_tokens=96, seed=7, force_stop=ENDS5, _trace=trace,
                               **kw, **GREEDY))
    return ev, trace


def test_five_utterances_through_two_slots_fp32_have_the_bits_of_the_repeated_pass(tts32, cond_mel, texts):
    """Slots are refilled (three times) and their cache rows reset: a row that kept its predecessor's keys would not give these bits."""
    off, t0 = queue_events(tts32, cond_mel, texts)
    on, t1 = queue_events(tts32, cond_mel, texts, latent_cache=True)
    assert tts32.gpt.engine.refill_stats["rows_refilled"] == 3
    assert sorted(t1["codes"]) == list(range(5)) and all(torch.equal(t0["codes"][u], t1["codes"][u]) for u in range(5))
    assert t0["frames"] == t1["frames"]
    same_events(on, off)


def test_five_utterances_through_two_slots_16bit_hold_the_stream_bound(tts16, cond_mel, texts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wavs, rows = tts16.infer_queue(cond_mel, texts, slots=2, max_mel_tokens=96, force_stop=ENDS5, seed=7, return_codes=True,
                                       check_every=CHUNK, **GREEDY)
    on, trace = queue_events(tts16, cond_mel, texts, latent_cache=True)
    for u in range(5):
        assert torch.equal(trace["codes"][u], rows[u].long().cpu())
        got = torch.cat([p for h, p, _ in on if h == u])
        rms = rel_rms(got, wavs[u])
        print(f"stream latent cache | bf16 | queue utterance {u}, {ENDS5[u]} frames | waveform rms against infer_queue = {rms:.3e}")
        assert got.shape == wavs[u].shape and rms <= RMS_16BIT, rms


# ---------------------------------------------------------------------------------------------------------------- front ends
def test_front_ends_pass_the_keyword_through(tmp_path):
    import os

    from starlette.testclient import TestClient

    import api as itts_api
    import test_configs_gpu as cfgs
    from indextts.infer import IndexTTS
    tmp = str(tmp_path)
    prompt = cfgs._model_dir(tmp)
    tts = IndexTTS(cfg_path=os.path.join(tmp, "config.yaml"), model_dir=tmp, is_fp16=True)
    text = "你好世界, HELLO WORLD. 今天天气很好!"
    sents = tts.tokenizer.split_sentences(tts.tokenizer.tokenize(text), 10)
    kw = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.3, repetition_penalty=10.0, length_penalty=0.0, num_beams=1,
              max_mel_tokens=12, seed=7)
    seen = []
    real = tts._latents_incremental
    tts._latents_incremental = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = list(tts.infer_stream(prompt, text, 10, chunk_tokens=4, latent_cache=True, **kw))
        assert seen
        cond = tts._prompt(prompt)
        want = []
        for s in sents:
            ids = torch.tensor(tts.tokenizer.convert_tokens_to_ids(s), dtype=torch.int32)
            want += list(tts.stream_utterance(cond, ids, chunk_tokens=4, latent_cache=True, **kw))
        assert len(got) == len(want) >= 2 and all(torch.equal(a[1], b) for a, b in zip(got, want))
        app = itts_api.create_app(tts, model_dir=tmp, config_path=os.path.join(tmp, "config.yaml"), finetune_dir=os.path.join(tmp, "ft"),
                                  output_dir=os.path.join(tmp, "out"), stream_latent_cache=True)
        del seen[:]
        r = TestClient(app).post("/tts/stream", json=dict(text=text, prompt_audio_path=prompt, seed=7, max_mel_tokens=12,
                                                          max_text_tokens_per_sentence=10))
        assert r.status_code == 200, r.text
        assert seen                                                         # the route ran the incremental pass
        direct = torch.cat([p for _, p in tts.infer_stream(prompt, text, 10, latent_cache=True, **kw)])
        assert r.content == direct.float().cpu().numpy().astype("<i2").tobytes()
