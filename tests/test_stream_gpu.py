"""Streaming synthesis on the GPU (GPTEngine.decode_chunks, BigVGAN.vocode_window, IndexTTS.stream_utterance / infer_stream, /tts/stream)
against the whole-utterance path on the same weights: the 2-layer full-width synthetic model, one utterance, chunks of 8 tokens.

Bounds.  The streamed and the whole-utterance paths run the same kernels on the same values; a chunk's latent pass and vocoder
window have other row counts than the whole run's, so a launch may take another kernel form (another summation order).  fp32:
each path is within the project's fp32 bounds of the oracle (tests/test_engines_gpu.py: latent < 1e-3 max-abs, waveform <= 1e-4 RMS),
so the two are within TWICE those of each other (triangle inequality): latent < 2e-3, waveform <= 2e-4 RMS.  Benched precision
(bf16 GPT, fp16 vocoder): twice the fp16-vs-fp32 vocoder tolerance of test_bigvgan_half_tracks_fp32 (5e-3 RMS): 1e-2.
Measured on an MI355X: profiles/stream_parity.txt (`-s` prints the lines)."""
import numpy as np
import pytest
import torch

import synth
import weights
from refill_voices import make_factors

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMPLE = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1)
GREEDY = dict(do_sample=False, repetition_penalty=10.0, num_beams=1)
SILENT, STOP = 52, 8193
CHUNK = 8
T_CODES = 40        # code tests: the stop token after 40 codes (five boundaries, the stop inside the sixth burst)
T_AUDIO = 88        # audio tests: > left + right + 1 = 71 frames, so that windows lie inside the utterance, clipped at neither end


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
    return [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (12, 5, 17, 9)]


def prefill(tts, cond_mel, rows, max_new):
    """The prompt of `rows` in the engine, as _batch_tokens puts it there."""
    conds, _ = tts._prompt_features(cond_mel)
    L = max(int(t.numel()) for t in rows)
    batch = torch.full((len(rows), L), tts.cfg.gpt.stop_text_token, dtype=torch.int32)
    for i, t in enumerate(rows):
        batch[i, : t.numel()] = t
    emb, pad = tts.gpt.prefix_rows(conds, batch)
    tts.gpt.engine.prefill(emb, pad, max_new, shared_rows=int(conds.shape[1]))
    return conds


def few_silent(codes):
    return int((codes == SILENT).sum()) <= 30


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("B", [4, 1])
@pytest.mark.parametrize("gen", [GREEDY, SAMPLE], ids=["greedy", "sampling"])
def test_bursts_equal_the_whole_loop(tts32, cond_mel, texts, B, gen):
    from indextts.gpt.model import sampling_params
    eng = tts32.gpt.engine
    rows, stops = texts[:B], [T_CODES, 17, 33, 9][:B]
    g, _ = tts32._gen_kwargs(dict(gen))
    sp = sampling_params(g, 21)
    prefill(tts32, cond_mel, rows, 48)
    want = eng.decode(48, dict(sp), force_stop=stops)
    graphs = len(eng._graphs)
    assert graphs >= 1
    prefill(tts32, cond_mel, rows, 48)
    seen = []
    for codes, fin in eng.decode_chunks(48, dict(sp), CHUNK, force_stop=stops):
        assert codes.dtype == torch.int64 and not codes.is_cuda and fin.shape == (B,)
        seen.append((codes, fin))
    assert [c.shape[1] for c, _ in seen] == [8, 16, 24, 32, 40, 48]          # a boundary every CHUNK tokens, token 1 included
    assert torch.equal(seen[-1][0], want.cpu())
    for codes, fin in seen:                                                 # every burst is a prefix, the flags say who has stopped
        n = codes.shape[1]
        assert torch.equal(codes, want.cpu()[:, :n])
        assert fin.tolist() == [bool((want[b, :n] == STOP).any()) for b in range(B)]
    assert bool(seen[-1][1].all())
    assert len(eng._graphs) == graphs                                       # the step decode() captured was replayed, none added
    for b, s in enumerate(stops):
        assert (want[b, :s] != STOP).all() and (want[b, s:] == STOP).all()


# ---------------------------------------------------------------------------------------------------------------- 2
def stream(tts, cond_mel, text, T, seed=5, gen=SAMPLE, **kw):
    trace = {}
    chunks = list(tts.stream_utterance(cond_mel, text, chunk_tokens=CHUNK, max_mel_tokens=T + 2 * CHUNK, seed=seed, force_stop=[T],
                                       _trace=trace, **kw, **gen))
    return chunks, trace


def batch(tts, cond_mel, text, T, seed=5, gen=SAMPLE, **kw):
    wavs, rows = tts.infer_batch(cond_mel, [text], max_mel_tokens=T + 2 * CHUNK, force_stop=[T], seed=seed, return_codes=True, **kw, **gen)
    return wavs[0], rows[0].long().cpu()


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_streamed_codes_equal_the_batch_codes(tts32, tts16, cond_mel, texts, which):
    tts = tts32 if which == "fp32" else tts16
    _, want = batch(tts, cond_mel, texts[0], T_CODES)
    assert want.numel() == T_CODES and few_silent(want)      # the condition under which the stream's silence rule is the identity
    chunks, trace = stream(tts, cond_mel, texts[0], T_CODES)
    assert torch.equal(trace["codes"], want)
    assert trace["frames"] == [(0, 5), (5, 40)]              # k = 40 codes known: 40 - right; then the flush at the stop token
    assert [int(c.numel()) for c in chunks] == [5 * 1024, 35 * 1024]


# ---------------------------------------------------------------------------------------------------------------- 3
def test_interleaved_passes_disturb_nothing(tts16, cond_mel, texts):
    """A latent pass and a vocoder run after EVERY burst (from the first on, whatever the halo): the loop's later tokens are those
    of the uninterrupted loop.  Fails if the interleaved passes write a buffer the decode step reads."""
    from indextts.gpt.model import sampling_params
    tts, eng, text = tts16, tts16.gpt.engine, texts[0]
    g, _ = tts._gen_kwargs(dict(SAMPLE))
    sp = sampling_params(g, 9)
    conds = prefill(tts, cond_mel, [text], 48)
    want = eng.decode(48, dict(sp), force_stop=[T_CODES]).cpu()
    prefill(tts, cond_mel, [text], 48)
    spk = tts._prompt_features(cond_mel)[1]
    ran = 0
    for codes, fin in eng.decode_chunks(48, dict(sp), CHUNK, force_stop=[T_CODES]):
        n = codes.shape[1]
        assert torch.equal(codes, want[:, :n]), n
        if not bool(fin[0]):
            lat = tts._latents(conds, [text], [codes[0]], reuse_prefix=True)[0]
            wav = tts.bigvgan.vocode_window(lat, spk, 0, n)
            assert lat.shape[0] == n and wav.numel() == n * 1024 and bool(torch.isfinite(wav).all())
            ran += 1
    assert ran == 5 and torch.equal(codes, want)


# ---------------------------------------------------------------------------------------------------------------- 4, 5
def audio_parity(tts, cond_mel, text, tag):
    """(waveform RMS in [-1, 1] units, latent max-abs) between the streamed and the whole-utterance path, T_AUDIO frames."""
    want, codes = batch(tts, cond_mel, text, T_AUDIO)
    assert codes.numel() == T_AUDIO and few_silent(codes)
    chunks, trace = stream(tts, cond_mel, text, T_AUDIO)
    assert torch.equal(trace["codes"], codes)
    left, right = tts.bigvgan.receptive_halo()
    assert any(a > left for a, _ in trace["frames"][:-1])      # a window that begins inside the utterance and ends before its end
    got = torch.cat(chunks)
    assert got.shape == want.shape == (T_AUDIO * 1024,)        # exactly the whole utterance's length
    conds = tts._prompt_features(cond_mel)[0]
    whole = tts._latents(conds, [text], [codes], reuse_prefix=False)[0]
    lat_err = (torch.cat(trace["latent"]) - whole).abs().max().item()
    rms = ((got - want) / 32767.0).pow(2).mean().sqrt().item()
    print(f"stream parity | {tag} | {T_AUDIO} frames, chunks of {CHUNK} | waveform rms = {rms:.3e}  max-abs = "
          f"{((got - want) / 32767.0).abs().max().item():.3e}  latent max-abs = {lat_err:.3e}  chunks = {trace['frames']}")
    return rms, lat_err, got, want


def test_streamed_audio_equals_the_whole_utterance_fp32(tts32, cond_mel, texts, monkeypatch):
    rms, lat_err, _, want = audio_parity(tts32, cond_mel, texts[0], "fp32 GPT, fp32 vocoder")
    assert lat_err < 2e-3, lat_err
    assert rms <= 2e-4, rms
    # negative control: without the halo the same comparison leaves the bound (each window then ends at false edges)
    monkeypatch.setattr(tts32.bigvgan, "receptive_halo", lambda: (0, 0))
    chunks, trace = stream(tts32, cond_mel, texts[0], T_AUDIO)
    got = torch.cat(chunks)
    assert got.shape == want.shape and len(chunks) > 2
    rms0 = ((got - want) / 32767.0).pow(2).mean().sqrt().item()
    print(f"stream parity | fp32, halo (0, 0): negative control | waveform rms = {rms0:.3e}  chunks = {len(chunks)}")
    assert rms0 > 2e-4, rms0


def test_streamed_audio_equals_the_whole_utterance_benched_precision(tts16, cond_mel, texts):
    rms, lat_err, _, _ = audio_parity(tts16, cond_mel, texts[0], "bf16 GPT, fp16 vocoder")
    assert rms <= 2 * 5e-3, rms


# ---------------------------------------------------------------------------------------------------------------- 6
def test_stream_over_the_fp8_kv_cache(state, cond_mel, texts):
    tts = make_tts(state, "bf16", "fp16", kv_cache="fp8")
    assert tts.gpt.engine.kv_dtype is not None
    _, want = batch(tts, cond_mel, texts[0], T_CODES)
    assert few_silent(want)
    chunks, trace = stream(tts, cond_mel, texts[0], T_CODES)     # (the latent passes take the whole-sequence form: see _latents)
    assert torch.equal(trace["codes"], want) and sum(int(c.numel()) for c in chunks) == T_CODES * 1024


def test_stream_with_a_voice_of_the_bank(state, cond_mel, texts):
    tts = make_tts(state)
    tts.gpt.attach_lora_bank(make_factors(state[0], (4, 8, 16), (2.0, 1.0, 0.5)))
    wav, want = batch(tts, cond_mel, texts[0], T_CODES, adapter_ids=[1])
    assert few_silent(want)
    chunks, trace = stream(tts, cond_mel, texts[0], T_CODES, adapter_ids=[1])
    assert torch.equal(trace["codes"], want)
    got = torch.cat(chunks)
    assert got.shape == wav.shape and ((got - wav) / 32767.0).pow(2).mean().sqrt().item() <= 2e-4


# ---------------------------------------------------------------------------------------------------------------- 7
def test_callers_stream_sentence_by_sentence(tmp_path):
    import os
    import warnings

    from starlette.testclient import TestClient

    import api as itts_api
    import test_configs_gpu as cfgs
    from indextts.infer import IndexTTS
    tmp = str(tmp_path)
    prompt = cfgs._model_dir(tmp)
    tts = IndexTTS(cfg_path=os.path.join(tmp, "config.yaml"), model_dir=tmp, is_fp16=True)
    text = "你好世界, HELLO WORLD. 今天天气很好!"
    sents = tts.tokenizer.split_sentences(tts.tokenizer.tokenize(text), 10)      # (short sentences merge under a larger limit)
    assert len(sents) == 2
    kw = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.3, repetition_penalty=10.0, length_penalty=0.0, num_beams=1,
              max_mel_tokens=12, seed=7)
    with pytest.warns(RuntimeWarning):                         # max_mel_tokens is reached, and said, as infer() says it
        got = list(tts.infer_stream(prompt, text, 10, chunk_tokens=4, **kw))
    assert all(sr == 24000 for sr, _ in got)
    cond = tts._prompt(prompt)
    want = []
    for s in sents:
        ids = torch.tensor(tts.tokenizer.convert_tokens_to_ids(s), dtype=torch.int32)
        want += list(tts.stream_utterance(cond, ids, chunk_tokens=4, **kw))
    assert len(got) == len(want) >= 2 and all(torch.equal(a[1], b) for a, b in zip(got, want))
    pcm = torch.cat([c for _, c in got])
    assert pcm.numel() > 0 and pcm.numel() % 1024 == 0
    app = itts_api.create_app(tts, model_dir=tmp, config_path=os.path.join(tmp, "config.yaml"), finetune_dir=os.path.join(tmp, "ft"),
                              output_dir=os.path.join(tmp, "out"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = TestClient(app)
        r = c.post("/tts/stream", json=dict(text=text, prompt_audio_path=prompt, seed=7, max_mel_tokens=12, max_text_tokens_per_sentence=10))
        assert r.status_code == 200, r.text
        assert r.headers["content-type"].startswith("audio/L16") and "rate=24000" in r.headers["content-type"] and r.headers["x-seed"] == "7"
        direct = torch.cat([p for _, p in tts.infer_stream(prompt, text, 10, **kw)])
        assert r.content == direct.float().cpu().numpy().astype("<i2").tobytes()
        assert c.post("/tts/stream", json=dict(text=text)).status_code == 400
        assert c.post("/tts/stream", json=dict(text=text, prompt_audio_path=os.path.join(tmp, "nope.wav"))).status_code == 404


def test_cli_stream_writes_the_streamed_chunks(tmp_path):
    """`indextts ... --stream`: the file holds infer_stream's chunks (default settings, num_beams = 1), 24 kHz mono 16-bit."""
    import os
    import wave

    import test_configs_gpu as cfgs
    from indextts.cli import main as cli_main
    from indextts.infer import IndexTTS
    tmp = str(tmp_path)
    prompt = cfgs._model_dir(tmp)
    out, text = os.path.join(tmp, "sub", "gen.wav"), "你好世界. HELLO!"
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        with pytest.warns(RuntimeWarning):     # (random weights never emit the stop token: the limit of 600 codes is reached)
            cli_main([text, "-v", prompt, "-o", out, "-c", os.path.join(tmp, "config.yaml"), "--model_dir", tmp, "--stream"])
        with pytest.raises(SystemExit):        # the other flags keep their meaning: no overwrite without --force
            cli_main([text, "-v", prompt, "-o", out, "-c", os.path.join(tmp, "config.yaml"), "--model_dir", tmp, "--stream"])
    finally:
        os.chdir(cwd)
    with wave.open(out, "rb") as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (24000, 1, 2)
        got = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    tts = IndexTTS(cfg_path=os.path.join(tmp, "config.yaml"), model_dir=tmp, is_fp16=True)
    with pytest.warns(RuntimeWarning):
        want = torch.cat([p for _, p in tts.infer_stream(prompt, text)]).float().cpu().numpy().astype("int16")
    assert got.size == want.size > 0 and got.size % 1024 == 0 and np.array_equal(got, want)
