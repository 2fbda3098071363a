"""The streaming queue, the parts that need no GPU: IndexTTS._stream_queue driven by a scripted refill loop over a stub engine -- rows
with different starts are planned on their own counts, every utterance's windows tile it, one `last` each --, the refusals of
stream_queue come before anything is launched, late arrivals (`more`) are fed, held back or end the loop, and the REST opt-in
serves two overlapping /tts/stream requests from ONE loop."""
import itertools
import threading
import types

import pytest
import torch

STOP = 8193
HOP = 4          # samples per frame of the stub vocoder
CHUNK = 8
RIGHT = 35
GEN = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1, length_penalty=0.0)


def code(handle_text, t):
    """Code t of the utterance whose text begins with the token `handle_text`."""
    return 1000 * int(handle_text) + t


class StubQueueTTS:
    """Everything IndexTTS._stream_queue touches, on the host.  The engine's decode_refill_chunks is the refill loop's schedule,
    scripted: polls every `check_every` steps from n = 1, a fed row joins one poll after it was fed (staged) with start = n - 1,
    a row of T codes (its force_stop) stops at the first poll with k > T.  A text's first token names the utterance; a latent row
    holds its code's value and the vocoder repeats a frame's value HOP times."""
    device = "cpu"
    VOCODER_BUCKET_RATIO = 2.0

    def __init__(self, max_text_tokens=40):
        from indextts.infer import IndexTTS
        self.loops, self.records, self.feeds, self.latent_calls, self.closed_loops = 0, [], [], [], 0
        self.engine = types.SimpleNamespace(prefill=self.prefill, decode_refill_chunks=self.decode_refill_chunks, paged=True, kv=object(),
                                            bank=None, refill_leftover=[], _S=0)
        self.gpt = types.SimpleNamespace(stop_mel_token=STOP, engine=self.engine, prefix_rows=self.prefix_rows, max_text_tokens=max_text_tokens)
        self.cfg = types.SimpleNamespace(gpt=types.SimpleNamespace(stop_text_token=1))
        self.bigvgan = types.SimpleNamespace(receptive_halo=lambda: (RIGHT, RIGHT))
        self.stream_plan, self.stream_queue_plan = IndexTTS.stream_plan, IndexTTS.stream_queue_plan
        self._vocode_windows = types.MethodType(IndexTTS._vocode_windows, self)
        self._queue_request = types.MethodType(IndexTTS._queue_request, self)
        self._refill_loops = types.MethodType(IndexTTS._refill_loops, self)
        self.stream_queue = types.MethodType(IndexTTS.stream_queue, self)
        self._stream_queue = types.MethodType(IndexTTS._stream_queue, self)
        self.conditioned = []
        self.gpt.get_conditioning = self.get_conditioning
        self.bigvgan.speaker_embedding = lambda m: torch.zeros(1, 1, 4)

    def prefix_rows(self, conds, batch):
        """[n, 2 + L + 2, 3]; element [j, p, 0] names the utterance (its text's first token)"""
        n, L = batch.shape
        pad = torch.tensor([int((batch[j] == 1).sum()) for j in range(n)])
        emb = torch.zeros(n, 2 + L + 2, 3)
        for j in range(n):
            emb[j, :, 0] = float(batch[j, 0])
        return emb, pad

    def prefill(self, emb, pad, max_new, shared_rows=0, slots_window=0, **kw):
        self.first = [int(emb[j, -1, 0]) for j in range(emb.shape[0])]
        self.engine._S = emb.shape[1] + 1
        self.window = slots_window

    def decode_refill_chunks(self, max_new, sp, feed, force_stop=None, check_every=16, staged=True, closed=None, positions=None, **kw):
        self.loops += 1
        B, ce = len(self.first), check_every
        owner, start, T, name = list(range(B)), [0] * B, list(force_stop), list(self.first)
        ids, pending, fed_out, n = itertools.count(B), None, False, 1
        self.engine.refill_leftover = []
        try:
            while True:
                if pending is not None:
                    for r, t, nm in pending:
                        owner[r], start[r], T[r], name[r] = next(ids), n - 1, t, nm
                    pending = None
                free = [r for r in range(B) if owner[r] is None]
                items = []
                if free and not fed_out and n > 1:
                    items = list(feed(len(free)))
                    self.feeds.append((n, len(free), len(items)))
                    fed_out = len(items) < len(free) and (closed is None or bool(closed()))
                if (fed_out or closed is not None) and pending is None and not items and all(o is None for o in owner):
                    return
                n += ce
                if items:
                    pending = [(r, int(it[1]), int(it[0][-1, 0])) for r, it in zip(free, items)]
                    for r, _, _ in pending:
                        owner[r] = -1
                rows = []
                for r in range(B):
                    if owner[r] is None or owner[r] < 0:
                        continue
                    k = n - start[r]
                    c = torch.full((k,), STOP, dtype=torch.int64)
                    m = min(k, T[r])
                    c[:m] = torch.tensor([code(name[r], t) for t in range(m)], dtype=torch.int64)
                    rows.append({"utt": owner[r], "slot": r, "k": k, "codes": c, "stopped": k > T[r], "prompt": (r, 0, 1)})
                    if k > T[r]:
                        owner[r] = None
                self.records.append((n, [(row["utt"], row["k"]) for row in rows]))
                yield {"n": n, "rows": rows}
        finally:
            self.closed_loops += 1

    def _prompt_features(self, cond_mel):
        return torch.zeros(1, 2, 3), torch.zeros(1, 1, 4)

    def get_conditioning(self, mel, lengths):
        if mel.shape[-1] < 3:
            raise RuntimeError("prompt too short")
        self.conditioned.append(int(mel.shape[-1]))
        return torch.zeros(1, 2, 3)

    def _latents(self, conds, text_rows, code_rows, reuse_prefix=False, **kw):
        assert not reuse_prefix and len(text_rows) == len(code_rows)
        self.latent_calls.append([(int(t[0]), int(c.numel())) for t, c in zip(text_rows, code_rows)])
        return [c.float()[:, None].expand(-1, 2) for c in code_rows]

    def _vocode(self, x, spk, lens=None):
        return x[:, :, 0].repeat_interleave(HOP, dim=1)


def text_of(name, length):
    return torch.tensor([name] + [7] * (length - 1), dtype=torch.int32)


def run(names_lengths, ends, slots=2, more=None, limit=96, stub=None):
    """The utterances (name, text length) with `ends` codes each through IndexTTS._stream_queue over the stub."""
    from indextts.infer import IndexTTS
    from indextts.gpt.model import row_sampling_params
    stub, trace = stub or StubQueueTTS(), {}
    sampling = row_sampling_params([{}] * len(ends), len(ends), GEN, 7) if more is not None else [None] * len(ends)
    reqs = [dict(handle=i, text=text_of(nm, ln), prompt=0, stop=e, sp=sampling[i], voice=None)
            for i, ((nm, ln), e) in enumerate(zip(names_lengths, ends))]
    events = list(IndexTTS._stream_queue(stub, "mel", reqs, slots, CHUNK, limit, 7, None, more, trace, dict(GEN)))
    return events, trace, stub


def whole(name, T):
    return torch.tensor([code(name, t) for t in range(T)]).float().repeat_interleave(HOP)


def check_contract(events, trace, names, ends):
    for h, (nm, T) in enumerate(zip(names, ends)):
        fr = trace["frames"][h]
        assert fr[0][0] == 0 and fr[-1][1] == T and all(a[1] == c[0] for a, c in zip(fr, fr[1:])) and all(b > a for a, b in fr)
        mine = [(pcm, last) for u, pcm, last in events if u == h]
        assert [last for _, last in mine] == [False] * (len(mine) - 1) + [True]       # exactly one last, at the end
        assert torch.equal(torch.cat([p for p, _ in mine]), whole(nm, T))             # the frames [0, T), once, in order
        assert trace["codes"][h].tolist() == [code(nm, t) for t in range(T)]


# ---------------------------------------------------------------------------------------------------------------- planner
def test_rows_are_planned_on_their_own_counts():
    names, ends = [(10, 12), (11, 5), (12, 17), (13, 9), (14, 14)], [44, 60, 38, 75, 52]
    events, trace, stub = run(names, ends)
    check_contract(events, trace, [n for n, _ in names], ends)
    assert stub.loops == 1 and stub.closed_loops == 1 and trace["loops"] == 1
    assert stub.first == [12, 14]                                           # the longest texts start
    # utterance 2 (38 codes) stops at the poll n = 41; utterance 0 is fed there, joins at n = 49 (start 48), is first seen at n = 57
    assert trace["polls"][2] == list(range(9, 42, 8)) and trace["polls"][0][0] == 57
    assert trace["frames"][2] == [(0, 38)] and trace["frames"][4] == [(0, 6), (6, 14), (14, 52)]
    # its first chunk leaves at the first poll with k - right > 0: n = 89, k = 41
    assert trace["frames"][0] == [(0, 6), (6, 44)]
    first_emit = [c for c in stub.latent_calls if any(nm == 10 for nm, _ in c)][0]
    assert (10, 41) in first_emit
    assert trace["frames"][3] == [(0, 6), (6, 14), (14, 22), (22, 30), (30, 38), (38, 75)]
    # the rows that emit at a poll share ONE latent pass, each with its own count: at n = 41 slot 0's flush (38 codes) and slot 1's
    # first chunk (k = 41); at n = 89 utterance 0 alone (k = 41), utterance 3 beside it has k = 25 and is left out
    assert stub.latent_calls[0] == [(12, 38), (14, 41)] and [(10, 41)] in stub.latent_calls
    assert [u for u, _, _ in events[:2]] == [2, 4] and events[0][2] and not events[1][2]


def test_plan_of_one_poll():
    from indextts.infer import IndexTTS
    rows = [dict(utt=3, k=4, codes=torch.tensor([5, 6, STOP, STOP]), stopped=True),
            dict(utt=4, k=4, codes=torch.tensor([5, 6, 7, 8]), stopped=False),
            dict(utt=5, k=2, codes=torch.tensor([5, 6]), stopped=False)]
    plan = IndexTTS.stream_queue_plan(rows, {4: 1}, 1, 10, STOP)
    assert plan == [(3, 2, 0, 2, True), (4, 4, 1, 3, False), (5, 2, 0, 1, False)]
    assert IndexTTS.stream_queue_plan(rows[2:], {5: 1}, 1, 10, STOP) == []              # nothing new, not final: left out
    assert IndexTTS.stream_queue_plan(rows[1:2], {4: 3}, 1, 4, STOP) == [(4, 4, 3, 4, True)]   # k == max_mel_tokens: final


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_anything_is_launched():
    from indextts.infer import IndexTTS
    nobody = types.SimpleNamespace()                 # no model, no device: the checks need neither
    rows = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
    with pytest.raises(NotImplementedError, match="beam"):
        IndexTTS.stream_queue(nobody, None, rows, num_beams=3)
    with pytest.raises(ValueError, match="one of them"):
        IndexTTS.stream_queue(nobody, None, rows, adapter_ids=[0, 1], adapter_mix=[{0: 0.5}, None])
    with pytest.raises(ValueError, match="adapter_ids"):
        IndexTTS.stream_queue(nobody, None, rows, adapter_ids=[0])
    with pytest.raises(ValueError, match="adapter_mix"):
        IndexTTS.stream_queue(nobody, None, rows, adapter_mix=[{0: 0.5}] * 3)
    with pytest.raises(ValueError, match="sampling"):
        IndexTTS.stream_queue(nobody, None, rows, sampling=[{"seed": 1}])
    with pytest.raises(ValueError, match="force_stop"):
        IndexTTS.stream_queue(nobody, None, rows, force_stop=[3])
    with pytest.raises(ValueError, match="chunk_tokens"):
        IndexTTS.stream_queue(nobody, None, rows, chunk_tokens=0)
    with pytest.raises(ValueError, match="slots"):
        IndexTTS.stream_queue(nobody, None, rows, slots=0)
    with pytest.raises(TypeError, match="more"):
        IndexTTS.stream_queue(nobody, None, rows, more=[])
    with pytest.raises(TypeError, match="unknown generation settings"):
        IndexTTS.stream_queue(nobody, None, rows, beams=1)
    somebody = types.SimpleNamespace(gpt=types.SimpleNamespace(engine=types.SimpleNamespace(bank=None)))
    with pytest.raises(ValueError, match="prompts"):
        IndexTTS.stream_queue(somebody, [torch.zeros(1, 100, 9)], rows)
    with pytest.raises(ValueError, match="unknown keys"):
        IndexTTS.stream_queue(somebody, None, rows, sampling=[{"seed": 1}, {"beams": 2}])
    assert list(IndexTTS.stream_queue(somebody, None, [])) == []


# ---------------------------------------------------------------------------------------------------------------- more
def scripted_more(script):
    """more() that returns script[i] at its i-th call (a list, or None); calls are counted."""
    calls = []

    def more():
        calls.append(len(calls))
        i = len(calls) - 1
        return script[i] if i < len(script) else []
    return more, calls


def test_an_arrival_is_fed_at_the_next_free_slot_and_fully_emitted():
    late = dict(handle="late", text=text_of(15, 6), force_stop=50)
    more, calls = scripted_more([[], [], [late], [], None])            # boundary 2 = behind the poll n = 17; None at the call behind n = 33
    events, trace, stub = run([(10, 12), (12, 17)], [44, 38], more=more)
    assert len(calls) == 5 and stub.loops == 1                         # None was the last word: more() is not asked again
    check_contract(events, trace, [10, 12], [44, 38])
    # slot 1 (utterance 1, 38 codes) frees at n = 41: the arrival is fed there, joins at n = 49 and is first seen at n = 57
    assert (41, 1, 1) in stub.feeds and trace["polls"]["late"][0] == 57
    fr = trace["frames"]["late"]
    assert fr[0][0] == 0 and fr[-1][1] == 50 and all(a[1] == c[0] for a, c in zip(fr, fr[1:]))
    mine = [(pcm, last) for u, pcm, last in events if u == "late"]
    assert [last for _, last in mine] == [False] * (len(mine) - 1) + [True]
    assert torch.equal(torch.cat([p for p, _ in mine]), whole(15, 50))


def test_an_over_long_arrival_is_held_for_the_next_loop():
    """The pool is sized for the longest prompt the model takes (max_text_tokens = 40 here): a text of 50 tokens does not fit the
    running loop's windows.  Nothing is raised: the arrival waits, a later and shorter one passes it, and it starts the next loop."""
    long_ = dict(handle="long", text=text_of(16, 50), force_stop=40)
    short = dict(handle="short", text=text_of(17, 6), force_stop=37)
    more, calls = scripted_more([[], [long_], [short], None])
    events, trace, stub = run([(10, 12), (12, 17)], [44, 38], more=more)
    assert stub.loops == 2 and trace["loops"] == 2 and stub.closed_loops == 2
    check_contract(events, trace, [10, 12], [44, 38])
    order = [u for u, _, last in events if last]
    assert order.index("short") < order.index("long")
    for h, nm, T in (("long", 16, 40), ("short", 17, 37)):
        assert torch.equal(torch.cat([p for u, p, _ in events if u == h]), whole(nm, T))
    assert stub.first == [16]                                           # the second loop was prefilled with it


def test_an_open_queue_that_falls_idle_ends_and_none_closes_it():
    # open and idle: more() never says None, the queue drains, the generator ends (the caller starts the next loop)
    more, calls = scripted_more([])
    events, trace, stub = run([(10, 12)], [20], slots=2, more=more)
    assert stub.loops == 1 and [u for u, _, last in events if last] == [0]
    n_calls = len(calls)
    assert n_calls >= 4                                                 # asked at every boundary, to the end
    # "no more will come" while rows are live: the feed is closed from then on, the rows run to their ends
    more, calls = scripted_more([[], None])
    events, trace, stub = run([(10, 12), (12, 17), (13, 9)], [44, 38, 40], slots=2, more=more)
    assert len(calls) == 2 and stub.loops == 1
    check_contract(events, trace, [10, 12, 13], [44, 38, 40])
    # nothing queued and nothing arriving: no loop at all
    more, calls = scripted_more([None])
    events, trace, stub = run([], [], more=more)
    assert events == [] and stub.loops == 0 and len(calls) == 1


def test_infer_stream_routes_through_the_queue_when_slots_is_given():
    from indextts.infer import IndexTTS
    seen = {}

    class Stub:
        tokenizer = types.SimpleNamespace(tokenize=lambda text: text.split(), split_sentences=lambda toks, limit: [[t] for t in toks],
                                          convert_tokens_to_ids=lambda sent: [int(t) for t in sent])

        def _prompt(self, path):
            return "mel of " + path

        def stream_queue(self, cond_mel, rows, slots=None, **kw):
            seen.update(cond_mel=cond_mel, rows=[int(r[0]) for r in rows], slots=slots, kw=kw)
            chunk = lambda s, i: torch.full((2,), 10.0 * s + i)      # noqa: E731
            for utt, i, last in [(2, 0, False), (0, 0, False), (1, 0, True), (2, 1, True), (0, 1, True)]:
                yield utt, chunk(utt, i), last

        def stream_utterance(self, *a, **k):
            raise AssertionError("slots was given: the sentences go through the queue")
        stream_batch = stream_utterance
    got = list(IndexTTS.infer_stream(Stub(), "p.wav", "0 1 2", slots=2, chunk_tokens=4, force_stop=[12]))
    assert seen["cond_mel"] == "mel of p.wav" and seen["rows"] == [0, 1, 2] and seen["slots"] == 2
    assert seen["kw"] == dict(chunk_tokens=4, force_stop=[12, 12, 12])
    assert [float(p[0]) for _, p in got] == [0.0, 1.0, 10.0, 20.0, 21.0] and all(sr == 24000 for sr, _ in got)   # text order
    with pytest.raises(ValueError, match="slots"):
        list(IndexTTS.infer_stream(Stub(), "p.wav", "0 1 2", slots=0))


# ---------------------------------------------------------------------------------------------------------------- service form
class StubServiceTTS(StubQueueTTS):
    """StubQueueTTS with what IndexTTS.serve_stream_queue adds: prompt files and a tokenizer (a word is a sentence of one token)."""

    def __init__(self):
        from indextts.infer import IndexTTS
        super().__init__()
        self.mels = {"ok.wav": torch.zeros(1, 100, 9), "short.wav": torch.zeros(1, 100, 2)}
        self.tokenizer = types.SimpleNamespace(tokenize=lambda text: text.split(), split_sentences=lambda toks, limit: [[t] for t in toks],
                                               convert_tokens_to_ids=lambda sent: [int(t) for t in sent])
        self.serve_stream_queue = types.MethodType(IndexTTS.serve_stream_queue, self)

    def _prompt(self, path):
        if path not in self.mels:
            raise FileNotFoundError(path)
        return self.mels[path]


def test_the_service_form_isolates_every_request():
    """The real serve_stream_queue over the stub engine: two requests interleave in one loop and each gets its own sentences in text
    order; a refused setting, an unreadable prompt, a prompt the conditioner refuses (found inside the queue) and a text without a
    sentence are each answered to their own request, and the others' audio arrives complete."""
    stub = StubServiceTTS()
    a = dict(handle="a", audio_prompt="ok.wav", text="21 22", max_mel_tokens=61, seed=7)
    b = dict(handle="b", audio_prompt="ok.wav", text="23", max_mel_tokens=45, temperature=0.7)
    cold = dict(handle="cold", audio_prompt="ok.wav", text="24", temperature=0.0)
    lost = dict(handle="lost", audio_prompt="missing.wav", text="25")
    mute = dict(handle="mute", audio_prompt="ok.wav", text="")
    short = dict(handle="short", audio_prompt="short.wav", text="26 27", max_mel_tokens=41)
    more, calls = scripted_more([[a, cold, lost, mute, b], [], [short], [], None])
    events = list(stub.serve_stream_queue(more, slots=3, chunk_tokens=CHUNK, max_mel_tokens=96))
    lasts = {}
    for h, pcm, last in events:
        if last:
            assert h not in lasts, h                                    # exactly one last per request
            lasts[h] = pcm
        else:
            assert h not in lasts and torch.is_tensor(pcm), h           # nothing behind a request's last
    assert sorted(lasts) == ["a", "b", "cold", "lost", "mute", "short"]
    assert isinstance(lasts["cold"], ValueError) and "temperature" in str(lasts["cold"])
    assert isinstance(lasts["lost"], FileNotFoundError)
    assert isinstance(lasts["short"], RuntimeError) and "too short" in str(lasts["short"])
    assert torch.is_tensor(lasts["mute"]) and lasts["mute"].numel() == 0
    audio = lambda h: torch.cat([p for u, p, _ in events if u == h and torch.is_tensor(p)])      # noqa: E731
    assert torch.equal(audio("a"), torch.cat([whole(21, 60), whole(22, 60)]))      # both sentences, in text order, complete
    assert torch.equal(audio("b"), whole(23, 44))
    assert stub.loops == 1 and stub.first == [21, 22, 23]               # one loop for both requests
    assert stub.conditioned == [9]                                      # the good prompt was conditioned once for all its requests
    order = [u for u, p, last in events if not last]
    assert order[:4] == ["a", "b", "a", "b"]          # the requests' chunks interleave; a's second sentence waits for its first


def test_a_default_prompt_the_call_does_not_have_is_refused():
    from indextts.infer import IndexTTS
    stub = StubQueueTTS()
    more, calls = scripted_more([[dict(handle="x", text=text_of(15, 6))], None])
    with pytest.raises(ValueError, match="prompt 0"):
        list(IndexTTS.stream_queue(stub, None, [], more=more))
    assert stub.loops == 0


# ---------------------------------------------------------------------------------------------------------------- REST
class StubService:
    """An engine for the REST routes that needs no device.  serve_stream_queue: every request is answered with three chunks that
    hold its own text's number; the loop waits (with a timeout, never reached) until two requests are in before it answers, so
    that two overlapping requests are provably served by one loop.  infer_stream: today's per-request call."""

    def __init__(self, expect=2):
        self.loops, self.alone, self.expect, self.slots = 0, 0, expect, None

    def chunks(self, text):
        return [torch.arange(4, dtype=torch.float32) + 100.0 * i + 1000.0 * int(text) for i in range(3)]

    def infer_stream(self, prompt, text, limit, **kw):
        self.alone += 1
        for c in self.chunks(text):
            yield 24000, c

    def serve_stream_queue(self, more, slots=32, **kw):
        self.loops += 1
        self.slots = slots
        live, waited = [], 0
        while len(live) < self.expect and waited < 2000:
            live += more()
            if len(live) < self.expect:
                threading.Event().wait(0.005)
                waited += 1
        for r in live:
            if r["text"] == "13":
                yield r["handle"], RuntimeError("refused setting"), True
        live = [r for r in live if r["text"] != "13"]
        for i in range(3):                               # interleaved: a chunk of each request in turn
            for r in live:
                assert r["audio_prompt"].endswith("p.wav") and r["seed"] == 7
                yield r["handle"], self.chunks(r["text"])[i], False
        for r in live:
            yield r["handle"], torch.zeros(0), True


def rest_client(tmp_path, eng, **kw):
    import os

    from starlette.testclient import TestClient

    import api as itts_api
    tmp = str(tmp_path)
    prompt = os.path.join(tmp, "p.wav")
    open(prompt, "wb").write(b"RIFF")
    app = itts_api.create_app(eng, model_dir=tmp, config_path=os.path.join(tmp, "config.yaml"), output_dir=os.path.join(tmp, "out"), **kw)
    return TestClient(app), prompt


def bytes_of(eng, text):
    import numpy as np
    return np.concatenate([c.numpy() for c in eng.chunks(text)]).astype("<i2").tobytes()


def test_rest_opt_in_serves_overlapping_streams_from_one_loop(tmp_path):
    eng = StubService(expect=2)
    c, prompt = rest_client(tmp_path, eng, stream_slots=4)
    out = {}

    def post(text):
        out[text] = c.post("/tts/stream", json=dict(text=text, prompt_audio_path=prompt, seed=7))
    threads = [threading.Thread(target=post, args=(t,)) for t in ("11", "12")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert eng.loops == 1 and eng.alone == 0 and eng.slots == 4          # ONE loop served both
    for text in ("11", "12"):
        r = out[text]
        assert r.status_code == 200 and r.content == bytes_of(eng, text) and r.headers["x-seed"] == "7"     # only its own bytes
        assert r.headers["content-type"].startswith("audio/L16")
    # a request that finds no loop starts one; what fails before its first chunk answers 500 and disturbs nobody
    eng.expect = 2
    threads = [threading.Thread(target=post, args=(t,)) for t in ("13", "14")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert eng.loops == 2
    assert out["13"].status_code == 500 and "refused setting" in out["13"].text
    assert out["14"].status_code == 200 and out["14"].content == bytes_of(eng, "14")
    assert c.post("/tts/stream", json=dict(text="15")).status_code == 400


def test_rest_opt_in_off_is_todays_route(tmp_path):
    eng = StubService()
    c, prompt = rest_client(tmp_path, eng)
    r = c.post("/tts/stream", json=dict(text="11", prompt_audio_path=prompt, seed=7))
    assert r.status_code == 200 and r.content == bytes_of(eng, "11")
    assert eng.alone == 1 and eng.loops == 0                             # infer_stream under the lock, as before
