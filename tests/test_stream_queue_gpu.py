"""The streaming queue on the GPU (GPTEngine.decode_refill_chunks, IndexTTS.stream_queue) against infer_queue on the same weights:
the 2-layer full-width synthetic model of tests/test_stream_batch_gpu.py, FIVE utterances through TWO slots, chunks (polls) of 8
tokens.  Texts of 12 / 5 / 17 / 9 / 14 tokens, forced stops after 44 / 60 / 38 / 75 / 52 codes.  The refilled loop polls at n = 1 + 8 j
(token 1 comes from the prefill logits, then whole blocks of 8 steps).  The longest texts enter first (utterances 2 and 4); slot 0
frees at the poll n = 41 and slot 1 at n = 57, so the two slots free at different polls and every refilled utterance joins while
the other slot is mid-stream (0 at n = 49, 3 at n = 65, 1 at n = 105).  Every utterance but the shortest (38 codes: no poll
falls between its 36th code and its stop) emits before its flush.

Bounds: those of tests/test_stream_gpu.py for the same comparison (streamed chunks against the whole-utterance waveform, RMS
error in [-1, 1] units; profiles/stream_parity.txt): fp32 2e-4, bf16 GPT / fp16 vocoder 2 * 5e-3 = 1e-2.  Codes are compared
exactly: the loop, its polls and its joins are infer_queue's."""
import hashlib
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
SLOTS, CHUNK = 2, 8
ENDS, LIMIT = [44, 60, 38, 75, 52], 96
RMS_FP32, RMS_16BIT = 2e-4, 2 * 5e-3            # tests/test_stream_gpu.py: tests 4 and 5 there
OWN_SEEDS = [dict(seed=3), dict(seed=4), dict(seed=5, temperature=0.7), dict(seed=6), dict(seed=7)]

# infer_queue(slots=2, check_every=8) of this queue on the commit BEFORE decode_refill became the drained generator (fp32, greedy,
# seed 7; one run on an MI355X): the engine's refill_stats and the sha1 of every utterance's codes (int64, little-endian)
PARENT_STATS = {"steps": 169, "polls": 21, "refill_calls": 3, "rows_refilled": 3, "staged": True, "blocks": 24, "peak_blocks": 20}
PARENT_SHA1 = ["766074b0584878f602ad74a91ceb918996c3783b", "d019d8e4a86630e4df44368fd387bb2b67d4f0ce",
               "6f1c1e071d500174ad350e2d91696adcad34a641", "39082669e45e64add3cb1ebb4c94d4d00d345ee9",
               "c8c28d90bd5288885ebb2c49c165e9405ff3e2ea"]


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


def hop_of(tts):
    return int(np.prod(tts.bigvgan.rates))


def whole(tts, cond_mel, texts, ends=ENDS, gen=GREEDY, **kw):
    """infer_queue: (waveforms, codes on the host)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wavs, rows = tts.infer_queue(cond_mel, texts, slots=SLOTS, max_mel_tokens=LIMIT, force_stop=ends, seed=7, return_codes=True,
                                     check_every=CHUNK, **kw, **gen)
    return wavs, [r.long().cpu() for r in rows]


def streamed(tts, cond_mel, texts, ends=ENDS, gen=GREEDY, **kw):
    """stream_queue: (events, trace), the contract of the events checked on the way."""
    trace = {}
    events = list(tts.stream_queue(cond_mel, texts, slots=SLOTS, chunk_tokens=CHUNK, max_mel_tokens=LIMIT, seed=7, force_stop=ends,
                                   _trace=trace, **kw, **gen))
    for u in trace["codes"]:
        lasts = [last for utt, _, last in events if utt == u]
        assert lasts == [False] * (len(lasts) - 1) + [True], (u, lasts)           # exactly one last per utterance, at its end
    return events, trace


def audio_of(events, u):
    return torch.cat([pcm for utt, pcm, _ in events if utt == u])


def few_silent(rows):
    return all(int((c == SILENT).sum()) <= 30 for c in rows)


def rel_rms(got, want):
    """RMS of the difference in [-1, 1] units, as tests/test_stream_gpu.py measures it."""
    return ((got - want) / 32767.0).pow(2).mean().sqrt().item()


_RUNS = {}


def pair(tts, tag, cond_mel, texts, gen, **kw):
    """One infer_queue and one stream_queue of the five utterances on `tts`, kept for the tests that read them: (waveforms, codes,
    events, trace, graphs after infer_queue, graphs after stream_queue, refill_stats of infer_queue's loop)."""
    if tag not in _RUNS:
        eng = tts.gpt.engine
        wavs, rows = whole(tts, cond_mel, texts, gen=gen, **kw)
        g0, stats = len(eng._graphs), dict(eng.refill_stats)
        events, trace = streamed(tts, cond_mel, texts, gen=gen, **kw)
        _RUNS[tag] = (wavs, rows, events, trace, g0, len(eng._graphs), stats)
    return _RUNS[tag]


def check_codes(tts, run):
    wavs, rows, events, trace, g0, g1, _ = run
    assert [int(r.numel()) for r in rows] == ENDS and few_silent(rows)     # (few silent tokens: the stream's silence rule is infer_queue's)
    assert sorted(trace["codes"]) == list(range(5)) and trace["loops"] == 1
    for u in range(5):
        assert torch.equal(trace["codes"][u], rows[u]), u
        assert audio_of(events, u).shape == wavs[u].shape == (ENDS[u] * hop_of(tts),)
        fr = trace["frames"][u]
        assert fr[0][0] == 0 and fr[-1][1] == ENDS[u] and all(a[1] == c[0] for a, c in zip(fr, fr[1:]))
    assert g0 >= 1 and g1 == g0                                            # the step infer_queue captured at B = 2 was replayed


# ---------------------------------------------------------------------------------------------------------------- codes
def test_codes_equal_infer_queue_fp32_greedy_and_no_graph_is_added(tts32, cond_mel, texts):
    run = pair(tts32, "fp32", cond_mel, texts, GREEDY)
    check_codes(tts32, run)
    trace = run[3]
    # utterances 2 and 4 (the longest texts) start; 0 joins at n = 49 in slot 0 while 4 is mid-stream, 3 at n = 65, 1 at n = 105
    assert trace["polls"][2] == list(range(9, 42, 8)) and trace["polls"][4] == list(range(9, 58, 8))
    assert trace["polls"][0][0] == 57 and trace["polls"][3][0] == 73 and trace["polls"][1][0] == 113
    assert trace["frames"][2] == [(0, 38)] and trace["frames"][4] == [(0, 6), (6, 14), (14, 52)]
    # a row that joined mid-loop is planned on its OWN count: utterance 0 has k = n - 48; its first chunk leaves at n = 89 (k = 41)
    assert trace["frames"][0] == [(0, 6), (6, 44)]
    assert trace["frames"][3] == [(0, 6), (6, 14), (14, 22), (22, 30), (30, 38), (38, 75)]


def test_codes_equal_infer_queue_bf16_with_a_seed_per_row(tts16, cond_mel, texts):
    check_codes(tts16, pair(tts16, "bf16", cond_mel, texts, SAMPLE, sampling=OWN_SEEDS))


def test_codes_equal_infer_queue_with_a_voice_per_utterance(state, cond_mel, texts):
    tts = make_tts(state, "bf16", "fp16")
    tts.gpt.attach_lora_bank(make_factors(state[0], (4, 8), (2.0, 1.0)))
    run = pair(tts, "bank", cond_mel, texts, SAMPLE, adapter_ids=[0, -1, 1, 0, 1])
    check_codes(tts, run)
    _, base = whole(tts, cond_mel, texts, gen=SAMPLE, adapter_ids=[-1] * 5)
    assert any(not torch.equal(a, c) for a, c in zip(base, run[1]))        # the voices were not ignored
    for u in range(5):
        assert rel_rms(audio_of(run[2], u), run[0][u]) <= RMS_16BIT, u


def test_codes_equal_infer_queue_over_the_fp8_kv_cache(state, cond_mel, texts):
    tts = make_tts(state, "bf16", "fp16", kv_cache="fp8")
    assert tts.gpt.engine.kv_dtype is not None
    run = pair(tts, "kv8", cond_mel, texts, SAMPLE)
    check_codes(tts, run)
    for u in range(5):
        assert bool(torch.isfinite(audio_of(run[2], u)).all())


# ---------------------------------------------------------------------------------------------------------------- chunks
def test_every_chunk_is_the_window_vocoded_alone_fp32(tts32, cond_mel, texts):
    """Every event's pcm equals BigVGAN.vocode_window -- that utterance alone, B = 1 -- (a) over the utterance's latents computed
    alone, by ONE single-row _latents call over all its codes after the stream has ended, and (b) over the latents its window was
    cut from (the trace's "window")."""
    wavs, rows, events, trace, _, _, _ = pair(tts32, "fp32", cond_mel, texts, GREEDY)
    conds, spk = tts32._prompt_features(cond_mel)
    for u in range(5):
        mine = [pcm for utt, pcm, _ in events if utt == u and pcm.numel()]
        assert len(mine) == len(trace["frames"][u]) == len(trace["window"][u])
        full = tts32._latents(conds, [texts[u]], [rows[u]], reuse_prefix=False)[0]
        for pcm, (t0, t1), (lo, win) in zip(mine, trace["frames"][u], trace["window"][u]):
            cut = torch.clamp(32767 * tts32.bigvgan.vocode_window(win, spk, t0 - lo, t1 - lo), -32767.0, 32767.0)
            alone = torch.clamp(32767 * tts32.bigvgan.vocode_window(full, spk, t0, t1), -32767.0, 32767.0)
            print(f"stream queue chunks | fp32 | utterance {u} frames [{t0}, {t1}) | max-abs vs the utterance alone = "
                  f"{(pcm - alone).abs().max().item():.3e}, vs its own window alone = {(pcm - cut).abs().max().item():.3e}")
            assert torch.equal(pcm, cut), (u, t0, t1)
            assert torch.equal(pcm, alone), (u, t0, t1)
        assert audio_of(events, u).numel() == hop_of(tts32) * ENDS[u]


# ---------------------------------------------------------------------------------------------------------------- audio
def parity(tts, tag, run, bound):
    wavs, rows, events, trace = run[:4]
    assert sum(len(trace["frames"][u]) > 1 for u in range(5)) >= 4  # chunks that end inside the utterance, on the halo alone
    for u in range(5):
        got = audio_of(events, u)
        assert got.shape == wavs[u].shape
        rms = rel_rms(got, wavs[u])
        print(f"stream queue parity | {tag} | utterance {u}, {ENDS[u]} frames, chunks {trace['frames'][u]} | waveform rms = {rms:.3e}")
        assert rms <= bound, (u, rms)
    return wavs


def test_audio_equals_infer_queue_fp32(tts32, cond_mel, texts, monkeypatch):
    wavs = parity(tts32, "fp32", pair(tts32, "fp32", cond_mel, texts, GREEDY), RMS_FP32)
    # negative control: without the halo a multi-chunk row leaves the bound (each window then ends at false edges)
    monkeypatch.setattr(tts32.bigvgan, "receptive_halo", lambda: (0, 0))
    events, trace = streamed(tts32, cond_mel, texts)
    worst = 0.0
    for u in range(5):
        assert len(trace["frames"][u]) > 2
        got = audio_of(events, u)
        assert got.shape == wavs[u].shape
        worst = max(worst, rel_rms(got, wavs[u]))
    print(f"stream queue parity | fp32, halo (0, 0): negative control | worst utterance rms = {worst:.3e}")
    assert worst > RMS_FP32, worst


def test_audio_equals_infer_queue_benched_precision(tts16, cond_mel, texts):
    parity(tts16, "bf16", pair(tts16, "bf16", cond_mel, texts, SAMPLE, sampling=OWN_SEEDS), RMS_16BIT)


# ---------------------------------------------------------------------------------------------------------------- engine
def test_the_drained_generator_is_the_parents_decode_refill(tts32, cond_mel, texts):
    wavs, rows, events, trace, _, _, stats = pair(tts32, "fp32", cond_mel, texts, GREEDY)
    assert stats == PARENT_STATS
    assert [hashlib.sha1(r.numpy().astype("<i8").tobytes()).hexdigest() for r in rows] == PARENT_SHA1
    assert dict(tts32.gpt.engine.refill_stats) == PARENT_STATS             # the generator's own loop (stream_queue ran last)


def engine_queue(tts, cond_mel, texts, sp, between=None):
    """The five utterances through GPTEngine.decode_refill_chunks as infer_queue sets the loop up: ({utt: codes}, records seen)."""
    g, eng = tts.gpt, tts.gpt.engine
    conds, _ = tts._prompt_features(cond_mel)
    order = sorted(range(5), key=lambda i: -int(texts[i].numel()))

    def prefixes(ids):
        L = max(int(texts[i].numel()) for i in ids)
        bh = torch.full((len(ids), L), tts.cfg.gpt.stop_text_token, dtype=torch.int32)
        for j, i in enumerate(ids):
            bh[j, : texts[i].numel()] = texts[i]
        return g.prefix_rows(conds, bh)
    first, rest = order[:SLOTS], order[SLOTS:]
    emb, pad = prefixes(first)
    eng.prefill(emb, pad, LIMIT + CHUNK + 1, shared_rows=int(conds.shape[1]), slots_window=emb.shape[1] + 1 + LIMIT + 2 * CHUNK + 2)
    entered, S, nc = list(first), int(emb.shape[1]) + 1, int(conds.shape[1])
    # where every prompt's keys lie: the prefilled rows behind their left padding; a row fed at the poll n joins at n + CHUNK,
    # its prompt + start token right in front of the join position S + n_join - 1 (_stage)
    first_pos = {i: int(eng._pad_host[j]) for j, i in enumerate(first)}
    seen_n = [1]

    def feed(k):
        take = [rest.pop(0) for _ in range(min(k, len(rest)))]
        if not take:
            return []
        e, p = prefixes(take)
        entered.extend(take)
        for i in take:
            first_pos[i] = S + (seen_n[0] + CHUNK) - 2 - (nc + int(texts[i].numel()) + 2)
        return [(e[j, p.tolist()[j]:], ENDS[i]) for j, i in enumerate(take)]
    codes, polls = {}, 0
    for rec in eng.decode_refill_chunks(LIMIT, dict(sp), feed, force_stop=[ENDS[i] for i in first], check_every=CHUNK, staged=True):
        polls += 1
        assert rec["n"] == 1 + CHUNK * polls
        for row in rec["rows"]:
            assert row["codes"].dtype == torch.int64 and not row["codes"].is_cuda and row["codes"].numel() == row["k"]
            slot, pos, length = row["prompt"]
            i = entered[row["utt"]]
            assert slot == row["slot"] and length == nc + int(texts[i].numel()) + 2 and pos == first_pos[i], (i, row["prompt"])
            if row["stopped"]:
                codes[entered[row["utt"]]] = row["codes"]
        seen_n[0] = rec["n"]
        if between is not None:
            between(rec, entered)
    assert not eng.refill_leftover
    return codes, polls


def test_interleaved_passes_disturb_nothing_beside_a_staged_prefill(tts16, cond_mel, texts):
    """A whole-sequence latent pass and a vocoder window after EVERY poll -- also the polls at which a refill's prefill has just
    been enqueued on the side stream -- leave every later token as it is in the uninterrupted loop."""
    from indextts.gpt.model import sampling_params
    tts = tts16
    g, _ = tts._gen_kwargs(dict(SAMPLE))
    sp = sampling_params(g, 9)
    want, polls = engine_queue(tts, cond_mel, texts, sp)
    conds, spk = tts._prompt_features(cond_mel)
    ran = []

    def between(rec, entered):
        rows = [r for r in rec["rows"] if not r["stopped"]]
        if rows:
            lats = tts._latents(conds, [texts[entered[r["utt"]]] for r in rows], [r["codes"] for r in rows], reuse_prefix=False)
            wav = tts.bigvgan.vocode_window(lats[0], spk, 0, int(lats[0].shape[0]))
            assert bool(torch.isfinite(wav).all()) and wav.numel() == rows[0]["k"] * hop_of(tts)
            ran.append(rec["n"])
    got, polls2 = engine_queue(tts, cond_mel, texts, sp, between)
    assert polls2 == polls and sorted(got) == sorted(want) == list(range(5))
    for u in range(5):
        assert torch.equal(got[u], want[u]), u
    assert {49, 65, 105}.issubset(ran)     # the polls behind a feed: _stage_beside had just been launched (stage D) when they ran


# ---------------------------------------------------------------------------------------------------------------- close
def test_a_closed_queue_leaves_the_engine_usable(state, tts32, cond_mel, texts):
    gen = tts32.stream_queue(cond_mel, texts, slots=SLOTS, chunk_tokens=CHUNK, max_mel_tokens=LIMIT, seed=7, force_stop=ENDS, **GREEDY)
    seen = [next(gen) for _ in range(3)]          # the poll n = 49: utterance 2 has flushed, utterance 0 is staged and has not joined
    assert [u for u, _, _ in seen] == [2, 4, 4] and seen[0][2] and not seen[1][2]
    gen.close()
    assert tts32.gpt.engine.kv.used_blocks() == 0
    kw = dict(max_mel_tokens=LIMIT, force_stop=ENDS[:4], seed=7, return_codes=True, **GREEDY)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wavs, rows = tts32.infer_batch(cond_mel, texts[:4], **kw)
        want_w, want_r = make_tts(state).infer_batch(cond_mel, texts[:4], **kw)
    for b in range(4):
        assert torch.equal(rows[b], want_r[b]) and torch.equal(wavs[b], want_w[b]), b


# ---------------------------------------------------------------------------------------------------------------- more
def test_a_late_arrival_is_streamed_completely(tts32, cond_mel, texts):
    """Utterance 1 (the shortest text: the static queue feeds it last) is handed in by `more` at the second boundary instead:
    it is fed in the same place, decodes the same codes and is streamed to its end under its handle."""
    per_row = [{}] * 5
    _, rows = whole(tts32, cond_mel, texts, sampling=per_row)
    calls = []

    def more():
        calls.append(len(calls))
        if len(calls) == 3:           # before the first prefill, after the poll n = 9, after the poll n = 17
            return [dict(handle="late", text=texts[1], force_stop=ENDS[1])]
        return None if len(calls) == 5 else []
    rest = [0, 2, 3, 4]
    events, trace = streamed(tts32, cond_mel, [texts[i] for i in rest], [ENDS[i] for i in rest], more=more)
    assert len(calls) == 5 and trace["loops"] == 1
    assert sorted(trace["codes"], key=str) == [0, 1, 2, 3, "late"]
    for j, i in enumerate(rest):
        assert torch.equal(trace["codes"][j], rows[i]), i
    assert torch.equal(trace["codes"]["late"], rows[1])
    assert trace["polls"]["late"][0] == 113 and trace["frames"]["late"][-1][1] == ENDS[1]
    assert audio_of(events, "late").numel() == hop_of(tts32) * ENDS[1]


def test_a_late_arrival_brings_its_own_prompt(tts32, cond_mel, texts):
    """The arrival names a prompt mel the call has not seen: its features are computed when it arrives, it speaks from its own
    prompt (the codes of infer_queue with a prompt per utterance), and the others are untouched."""
    other = torch.from_numpy(synth.uniform("stream.queue.cond_mel_b", (1, 100, 87), -6.0, 2.0)).to(DEV)
    prompts = [cond_mel, other, cond_mel, cond_mel, cond_mel]
    _, rows = whole(tts32, prompts, texts, sampling=[{}] * 5)
    _, same = whole(tts32, cond_mel, texts, sampling=[{}] * 5)
    assert not torch.equal(rows[1], same[1])                       # the prompt matters to utterance 1
    calls = []

    def more():
        calls.append(len(calls))
        if len(calls) == 3:
            return [dict(handle="late", text=texts[1], force_stop=ENDS[1], cond_mel=other)]
        return None if len(calls) == 5 else []
    rest = [0, 2, 3, 4]
    events, trace = streamed(tts32, cond_mel, [texts[i] for i in rest], [ENDS[i] for i in rest], more=more)
    for j, i in enumerate(rest):
        assert torch.equal(trace["codes"][j], rows[i]), i
    assert torch.equal(trace["codes"]["late"], rows[1])
    assert audio_of(events, "late").numel() == hop_of(tts32) * ENDS[1]
