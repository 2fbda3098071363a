"""Batched streaming on the GPU (IndexTTS.stream_batch) against the whole-utterance call on the same weights: the 2-layer full-width
synthetic model of tests/test_stream_gpu.py, four utterances in one token loop, chunks of 8 tokens.  The rows stop after 3 / 40 /
75 / 88 codes of at most 96, so that every branch of the per-row plan occurs: one flush shorter than the halo, a stop between two
boundaries, a mid-length row and a stop exactly on a boundary (88 = 11 * 8); with 64 codes at most and no stop in rows 2 and 3 the
token limit flushes.

Bounds: those of tests/test_stream_gpu.py for the same comparison (streamed chunks against infer_batch's waveform, RMS error in
[-1, 1] units): fp32 2e-4, bf16 GPT / fp16 vocoder 2 * 5e-3 = 1e-2; the reasoning is in that file's docstring."""
import warnings

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
ENDS, LIMIT = [3, 40, 75, 88], 96
RMS_FP32, RMS_16BIT = 2e-4, 2 * 5e-3            # tests/test_stream_gpu.py: tests 4 and 5 there


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


def hop_of(tts):
    return int(np.prod(tts.bigvgan.rates))


def whole(tts, cond_mel, texts, ends=ENDS, limit=LIMIT, seed=7, gen=GREEDY, **kw):
    """infer_batch: (waveforms, codes on the host)."""
    stops = [-1 if e is None else e for e in ends]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wavs, rows = tts.infer_batch(cond_mel, texts, max_mel_tokens=limit, force_stop=stops, seed=seed, return_codes=True, **kw, **gen)
    return wavs, [r.long().cpu() for r in rows]


def streamed(tts, cond_mel, texts, ends=ENDS, limit=LIMIT, seed=7, gen=GREEDY, **kw):
    """stream_batch: (events, trace), the contract of the events checked on the way."""
    trace = {}
    events = list(tts.stream_batch(cond_mel, texts, chunk_tokens=CHUNK, max_mel_tokens=limit, seed=seed, force_stop=ends, _trace=trace,
                                   **kw, **gen))
    for b in range(len(texts)):
        lasts = [last for row, _, last in events if row == b]
        assert lasts == [False] * (len(lasts) - 1) + [True], (b, lasts)           # exactly one last per row, at its end
    return events, trace


def audio_of(events, b):
    return torch.cat([pcm for row, pcm, _ in events if row == b])


def few_silent(rows):
    return all(int((c == SILENT).sum()) <= 30 for c in rows)


def rel_rms(got, want):
    """RMS of the difference in [-1, 1] units, as tests/test_stream_gpu.py measures it."""
    return ((got - want) / 32767.0).pow(2).mean().sqrt().item()


_RUNS = {}


def pair(tts, tag, cond_mel, texts, gen):
    """One infer_batch and one stream_batch of the four rows on `tts`, kept for the tests that read them: (waveforms, codes, events,
    trace, graphs after infer_batch, graphs after stream_batch)."""
    key = (tag, gen is SAMPLE)
    if key not in _RUNS:
        eng = tts.gpt.engine
        wavs, rows = whole(tts, cond_mel, texts, gen=gen)
        g0 = len(eng._graphs)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            events, trace = streamed(tts, cond_mel, texts, gen=gen)
        assert not any("max_mel_tokens" in str(w.message) for w in rec)     # every row meets its stop token: the limit is not mentioned
        _RUNS[key] = (wavs, rows, events, trace, g0, len(eng._graphs))
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------------------- 1, 8
@pytest.mark.parametrize("which,gen", [("fp32", GREEDY), ("bf16", GREEDY), ("bf16", SAMPLE)], ids=["greedy-fp32", "greedy-bf16", "sampling-bf16"])
def test_codes_equal_infer_batch_and_no_graph_is_added(tts32, tts16, cond_mel, texts, which, gen):
    tts = tts32 if which == "fp32" else tts16
    wavs, rows, events, trace, g0, g1 = pair(tts, which, cond_mel, texts, gen)
    assert [int(r.numel()) for r in rows] == ENDS and few_silent(rows)     # (few silent tokens: the stream's silence rule is infer_batch's)
    for b in range(4):
        assert torch.equal(trace["codes"][b], rows[b]), b
        assert audio_of(events, b).shape == wavs[b].shape == (ENDS[b] * hop_of(tts),)
    assert trace["frames"][0] == [(0, 3)] and trace["frames"][1] == [(0, 5), (5, 40)]
    assert trace["frames"][2] == [(0, 5), (5, 13), (13, 21), (21, 29), (29, 37), (37, 75)]
    assert trace["frames"][3] == [(0, 5), (5, 13), (13, 21), (21, 29), (29, 37), (37, 45), (45, 53), (53, 88)]
    assert trace["boundaries"] == [[8], list(range(8, 49, 8)), list(range(8, 81, 8)), list(range(8, 97, 8))]
    order = [row for row, _, _ in events]
    assert order == [0, 1, 2, 3, 1, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 3, 3]        # ascending rows within every boundary
    assert g0 >= 1 and g1 == g0                                               # the step decode() captured at B = 4 was replayed


# ---------------------------------------------------------------------------------------------------------------- 2
def test_every_chunk_is_the_window_vocoded_alone_fp32(tts32, cond_mel, texts):
    """Bit-equality of the ragged window path: every event's pcm equals BigVGAN.vocode_window -- that row alone, B = 1 -- (a) over
    the row's latents recomputed by ONE single-row _latents call after the stream has ended, and (b) over the latents its window
    was cut from (the trace's "window": the rows [lo, hi) of the boundary's batched latent pass).  (a) holds because, in fp32 at
    these shapes, the batched pass over k_b codes and the single pass over all T_b give the rows < k_b the same bits (measured
    on an MI355X: every window of every row); (b) holds by construction, whatever the latent pass rounds to."""
    wavs, rows, events, trace, _, _ = pair(tts32, "fp32", cond_mel, texts, GREEDY)
    conds, spk = tts32._prompt_features(cond_mel)
    for b in range(4):
        mine = [pcm for row, pcm, _ in events if row == b]
        assert len(mine) == len(trace["frames"][b]) == len(trace["window"][b])
        full = tts32._latents(conds, [texts[b]], [rows[b]], reuse_prefix=False)[0]
        for pcm, (t0, t1), (lo, win) in zip(mine, trace["frames"][b], trace["window"][b]):
            alone = torch.clamp(32767 * tts32.bigvgan.vocode_window(full, spk, t0, t1), -32767.0, 32767.0)
            assert torch.equal(pcm, alone), (b, t0, t1)
            cut = torch.clamp(32767 * tts32.bigvgan.vocode_window(win, spk, t0 - lo, t1 - lo), -32767.0, 32767.0)
            assert torch.equal(pcm, cut), (b, t0, t1)


# ---------------------------------------------------------------------------------------------------------------- 3
def parity(tts, tag, cond_mel, texts, gen, bound):
    wavs, rows, events, trace, _, _ = pair(tts, tag, cond_mel, texts, gen)
    left, right = tts.bigvgan.receptive_halo()
    assert any(a > left for a, _ in trace["frames"][3][:-1])        # a window inside the utterance, clipped at neither end
    for b in range(4):
        got = audio_of(events, b)
        assert got.shape == wavs[b].shape
        rms = rel_rms(got, wavs[b])
        print(f"stream batch parity | {tag} | row {b}, {ENDS[b]} frames, chunks {trace['frames'][b]} | waveform rms = {rms:.3e}")
        assert rms <= bound, (b, rms)
    return wavs


def test_audio_equals_the_whole_utterance_fp32(tts32, cond_mel, texts, monkeypatch):
    wavs = parity(tts32, "fp32", cond_mel, texts, GREEDY, RMS_FP32)
    # negative control: without the halo a multi-chunk row leaves the bound (each window then ends at false edges)
    monkeypatch.setattr(tts32.bigvgan, "receptive_halo", lambda: (0, 0))
    events, trace = streamed(tts32, cond_mel, texts)
    worst = 0.0
    for b in (1, 2, 3):
        assert len(trace["frames"][b]) > 2
        got = audio_of(events, b)
        assert got.shape == wavs[b].shape
        worst = max(worst, rel_rms(got, wavs[b]))
    print(f"stream batch parity | fp32, halo (0, 0): negative control | worst multi-chunk row rms = {worst:.3e}")
    assert worst > RMS_FP32, worst


def test_audio_equals_the_whole_utterance_benched_precision(tts16, cond_mel, texts):
    parity(tts16, "bf16", cond_mel, texts, SAMPLE, RMS_16BIT)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_a_row_streams_as_it_streams_alone(tts32, cond_mel, texts):
    wavs, rows, events, trace, _, _ = pair(tts32, "fp32", cond_mel, texts, GREEDY)
    alone = {}
    chunks = list(tts32.stream_utterance(cond_mel, texts[2], chunk_tokens=CHUNK, max_mel_tokens=LIMIT, seed=7, force_stop=[ENDS[2]],
                                         _trace=alone, **GREEDY))
    assert alone["frames"] == trace["frames"][2]
    assert [int(c.numel()) for c in chunks] == [int(p.numel()) for row, p, _ in events if row == 2]
    assert torch.equal(alone["codes"], rows[2])            # greedy: the row alone decodes what it decodes in the batch
    rms = rel_rms(torch.cat(chunks), audio_of(events, 2))
    print(f"stream batch parity | fp32 | row 2 of the batch against stream_utterance alone | waveform rms = {rms:.3e}")
    assert rms <= RMS_FP32, rms


@pytest.mark.parametrize("latent_cache", [False, True], ids=["repeated", "latent-cache"])
@pytest.mark.parametrize("which,gen", [("fp32", GREEDY), ("bf16", SAMPLE)], ids=["greedy-fp32", "sampling-bf16"])
def test_one_utterance_is_the_batch_of_one_row(tts32, tts16, cond_mel, texts, which, gen, latent_cache):
    """stream_utterance is stream_batch with the one row, unwrapped: the same chunks bit for bit, the same frames and codes.  17 text
    tokens, a stop after 40 codes of at most 48, chunks of 8: the boundary n = 40 is an interior one and emits (0, 5) from a window
    clipped on the left only, and the stop token, found at n = 48, flushes the rest."""
    tts = tts32 if which == "fp32" else tts16
    kw = dict(chunk_tokens=CHUNK, max_mel_tokens=48, seed=7, latent_cache=latent_cache, **gen)
    one, rows = {}, {}
    chunks = list(tts.stream_utterance(cond_mel, texts[2], force_stop=[40], _trace=one, **kw))
    events = list(tts.stream_batch(cond_mel, [texts[2]], force_stop=[40], _trace=rows, **kw))
    assert one["frames"] == rows["frames"][0] == [(0, 5), (5, 40)]
    assert torch.equal(one["codes"], rows["codes"][0]) and one["codes"].numel() == 40
    assert [(row, last) for row, _, last in events] == [(0, False), (0, True)]
    assert len(chunks) == 2 and all(torch.equal(c, pcm) for c, (_, pcm, _) in zip(chunks, events))
    assert torch.cat(chunks).numel() == 40 * hop_of(tts)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_prompt_voice_and_settings_per_row(state, texts):
    tts = make_tts(state)
    tts.gpt.attach_lora_bank(make_factors(state[0], (4, 8, 16), (2.0, 1.0, 0.5)))
    m0 = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    m1 = torch.from_numpy(synth.uniform("stream.batch.cond_mel_b", (1, 100, 87), -6.0, 2.0)).to(DEV)
    ends, limit = [3, 20, 41, 48], 56
    kw = dict(adapter_ids=[0, -1, 1, 0], sampling=[dict(seed=3), dict(seed=4), dict(seed=3, temperature=0.7), dict(seed=4)])
    prompts = [m0, m1, m1, m0]
    wavs, rows = whole(tts, prompts, texts, ends, limit, gen=SAMPLE, **kw)
    assert [int(r.numel()) for r in rows] == ends and few_silent(rows)
    events, trace = streamed(tts, prompts, texts, ends, limit, gen=SAMPLE, **kw)
    for b in range(4):
        assert torch.equal(trace["codes"][b], rows[b]), b
        got = audio_of(events, b)
        assert got.shape == wavs[b].shape
        rms = rel_rms(got, wavs[b])
        print(f"stream batch parity | fp32, a prompt, a voice and settings per row | row {b} | waveform rms = {rms:.3e}")
        assert rms <= RMS_FP32, (b, rms)
    assert len(trace["frames"][3]) > 1
    # the same four rows under ONE prompt and the base voice decode other codes: the lists above were not ignored
    _, base = whole(tts, m0, texts, ends, limit, gen=SAMPLE, adapter_ids=[-1] * 4, sampling=kw["sampling"])
    assert any(not torch.equal(a, c) for a, c in zip(base, rows))


# ---------------------------------------------------------------------------------------------------------------- 6
def test_stream_batch_over_the_fp8_kv_cache(state, cond_mel, texts):
    tts = make_tts(state, "bf16", "fp16", kv_cache="fp8")
    assert tts.gpt.engine.kv_dtype is not None
    ends, limit = [3, 20, 41, 48], 56
    wavs, rows = whole(tts, cond_mel, texts, ends, limit, gen=SAMPLE)
    assert few_silent(rows)
    events, trace = streamed(tts, cond_mel, texts, ends, limit, gen=SAMPLE)     # (the latent passes take the whole-sequence form)
    for b in range(4):
        assert torch.equal(trace["codes"][b], rows[b]), b
        got = audio_of(events, b)
        assert got.shape == (ends[b] * hop_of(tts),) and bool(torch.isfinite(got).all())


# ---------------------------------------------------------------------------------------------------------------- token limit
def test_token_limit_flushes_and_warns_per_row(tts16, cond_mel, texts):
    ends, limit = [3, 40, None, None], 64
    wavs, rows = whole(tts16, cond_mel, texts, ends, limit, gen=SAMPLE)
    assert [int(r.numel()) for r in rows] == [3, 40, 64, 64] and few_silent(rows)
    with pytest.warns(RuntimeWarning) as rec:
        events, trace = streamed(tts16, cond_mel, texts, ends, limit, gen=SAMPLE)
    assert sum("max_mel_tokens" in str(w.message) for w in rec) == 2            # rows 2 and 3, once each
    assert trace["frames"][2] == trace["frames"][3] == [(0, 5), (5, 13), (13, 21), (21, 64)]
    for b in range(4):
        assert torch.equal(trace["codes"][b], rows[b]), b
        rms = rel_rms(audio_of(events, b), wavs[b])
        assert rms <= RMS_16BIT, (b, rms)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_a_closed_stream_leaves_the_engine_usable(state, tts32, cond_mel, texts):
    gen = tts32.stream_batch(cond_mel, texts, chunk_tokens=CHUNK, max_mel_tokens=LIMIT, seed=7, force_stop=ENDS, **GREEDY)
    first = [next(gen), next(gen)]
    assert [row for row, _, _ in first] == [0, 1] and first[0][2] and not first[1][2]
    gen.close()
    wavs, rows = whole(tts32, cond_mel, texts)
    fresh = make_tts(state)
    want_w, want_r = whole(fresh, cond_mel, texts)
    for b in range(4):
        assert torch.equal(rows[b], want_r[b]) and torch.equal(wavs[b], want_w[b]), b


def test_sentences_in_parallel_are_the_batch_in_text_order(tts16, cond_mel, texts, monkeypatch):
    """infer_stream(parallel_sentences=4) over the real stream_batch: the chunks are those of the rows, row after row."""
    import types
    monkeypatch.setattr(tts16, "_prompt", lambda path: cond_mel)
    by_name = {f"s{i}": t for i, t in enumerate(texts)}
    monkeypatch.setattr(tts16, "tokenizer", types.SimpleNamespace(
        tokenize=lambda text: text.split(), split_sentences=lambda toks, limit: [[t] for t in toks],
        convert_tokens_to_ids=lambda sent: by_name[sent[0]].tolist()))
    kw = dict(chunk_tokens=CHUNK, max_mel_tokens=56, seed=7, **SAMPLE)
    ends = [3, 20, 41, 48]
    got = list(tts16.infer_stream("p.wav", "s0 s1 s2 s3", parallel_sentences=4, force_stop=ends, **kw))
    events = list(tts16.stream_batch(cond_mel, texts, force_stop=ends, **kw))
    want = [pcm for b in range(4) for row, pcm, _ in events if row == b and pcm.numel()]
    assert all(sr == 24000 for sr, _ in got)
    assert len(got) == len(want) and all(torch.equal(a, c) for (_, a), c in zip(got, want))
