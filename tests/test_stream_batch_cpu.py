"""Batched streaming, the parts that need no GPU: IndexTTS._stream_rows driven by recorded (codes, finished) polls over a stub
engine -- the per-row plan tiles every utterance, one `last` per row, the windows are cut where the plan says --, the refusals
of stream_batch come before anything is launched, and infer_stream(parallel_sentences=P) hands the chunks out in text order."""
import types
import warnings

import pytest
import torch

STOP = 8193
HOP = 4          # samples per frame of the stub vocoder
CHUNK = 8
GEN = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1, length_penalty=0.0)


def recorded_polls(ends, limit, chunk=CHUNK):
    """What GPTEngine.decode_chunks yields for rows that stop after ends[b] codes (None: never): codes [B, n] at every multiple of
    `chunk`, stop-token padded, until every row has stopped or n == limit.  Code t of row b is 1000 * b + t."""
    B = len(ends)
    full = torch.full((B, limit), STOP, dtype=torch.int64)
    for b, e in enumerate(ends):
        e = limit if e is None else e
        full[b, :e] = 1000 * b + torch.arange(e)
    polls, n = [], 0
    while True:
        n = min(n + chunk, limit)
        fin = (full[:, :n] == STOP).any(dim=1)
        polls.append((full[:, :n].clone(), fin))
        if bool(fin.all()) or n >= limit:
            return polls, full


class StubTTS:
    """Everything IndexTTS._stream_rows touches, on the host: the loop replays recorded polls, a latent row holds its code's
    value, and the vocoder repeats a frame's value HOP times -- so a chunk's samples say which frames it was cut from."""
    device = "cpu"
    VOCODER_BUCKET_RATIO = 2.0

    def __init__(self, polls, halo=(35, 35)):
        from indextts.infer import IndexTTS
        self.polls, self.latent_calls, self.vocoder_calls, self.prefills = polls, [], [], []
        self.closed = False
        eng = types.SimpleNamespace(prefill=lambda *a, **k: self.prefills.append((a, k)), decode_chunks=self.decode_chunks)
        self.gpt = types.SimpleNamespace(stop_mel_token=STOP, engine=eng,
                                         prefix_rows=lambda conds, batch: (torch.zeros(batch.shape[0], 3, 2), torch.zeros(batch.shape[0])))
        self.cfg = types.SimpleNamespace(gpt=types.SimpleNamespace(stop_text_token=1))
        self.bigvgan = types.SimpleNamespace(receptive_halo=lambda: halo)
        self.stream_plan, self.stream_batch_plan = IndexTTS.stream_plan, IndexTTS.stream_batch_plan
        self._vocode_windows = types.MethodType(IndexTTS._vocode_windows, self)      # the real bucketing and cutting

    def decode_chunks(self, max_new, sp, chunk, force_stop=None):
        try:
            for p in self.polls:
                yield p
        finally:
            self.closed = True

    def _prompt_features(self, cond_mel):
        return torch.zeros(1, 2, 2), torch.zeros(1, 1, 4)

    def _latents(self, conds, text_rows, code_rows, reuse_prefix=False, cache_rows=None, adapter_ids=None, adapter_mix=None):
        assert reuse_prefix and len(text_rows) == len(code_rows) == len(cache_rows)
        self.latent_calls.append((list(cache_rows), [int(c.numel()) for c in code_rows]))
        return [c.float()[:, None].expand(-1, 2) for c in code_rows]

    def _vocode(self, x, spk, lens=None):
        self.vocoder_calls.append((tuple(x.shape), lens))
        return x[:, :, 0].repeat_interleave(HOP, dim=1)


def run(ends, limit, halo=(35, 35), stop_after=None):
    from indextts.infer import IndexTTS
    polls, full = recorded_polls(ends, limit)
    stub, trace = StubTTS(polls, halo), {}
    texts = [torch.arange(3 + b, dtype=torch.int32) for b in range(len(ends))]
    gen = IndexTTS._stream_rows(stub, None, texts, CHUNK, limit, 7, None, None, None, None, trace, dict(GEN))
    events = []
    for ev in gen:
        events.append(ev)
        if stop_after is not None and len(events) == stop_after:
            gen.close()
            break
    return events, trace, stub, full


def test_every_branch_of_the_plan():
    ends = [3, 40, 75, 88]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # every row meets its stop token: nothing is said
        events, trace, stub, full = run(ends, 96)
    assert trace["frames"][0] == [(0, 3)]                                             # shorter than the halo: one flush
    assert trace["frames"][1] == [(0, 5), (5, 40)]                                    # the stop between two boundaries
    assert trace["frames"][2] == [(0, 5), (5, 13), (13, 21), (21, 29), (29, 37), (37, 75)]
    assert trace["frames"][3] == [(0, 5), (5, 13), (13, 21), (21, 29), (29, 37), (37, 45), (45, 53), (53, 88)]   # the stop ON a boundary
    for b, T in enumerate(ends):
        fr = trace["frames"][b]
        assert fr[0][0] == 0 and fr[-1][1] == T and all(a[1] == c[0] for a, c in zip(fr, fr[1:])) and all(t1 > t0 for t0, t1 in fr)
        mine = [(pcm, last) for row, pcm, last in events if row == b]
        assert [last for _, last in mine] == [False] * (len(mine) - 1) + [True]       # exactly one last, at the end
        assert len(mine) == len(fr)
        got = torch.cat([p for p, _ in mine])
        assert torch.equal(got, full[b, :T].float().repeat_interleave(HOP))           # the frames [0, T), once, in order
        assert torch.equal(trace["codes"][b], full[b, :T])
        assert torch.equal(torch.cat(trace["latent"][b])[:, 0], full[b, :T].float())
    # ascending rows within a boundary: n = 8 | 40 | 48 | 56 | 64 | 72 | 80 | 88 | 96
    assert [row for row, _, _ in events] == [0, 1, 2, 3, 1, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 3, 3]
    # one latent pass per boundary that emits, over the emitting rows only, each with the codes up to its own stop
    assert stub.latent_calls[0] == ([0], [3])
    assert stub.latent_calls[1] == ([1, 2, 3], [40, 40, 40])
    assert stub.latent_calls[2] == ([1, 2, 3], [40, 48, 48])
    assert stub.latent_calls[-1] == ([3], [88])
    assert len(stub.latent_calls) == 1 + 8                  # n = 8, then n = 40 .. 96
    # windows [max(0, t0 - 35), min(k, t1 + 35)): clipped at the utterance's start and at the codes known; ragged within a bucket
    assert stub.vocoder_calls == [((1, 3, 2), None), ((3, 40, 2), None), ((3, 48, 2), [40, 48, 48]), ((2, 56, 2), None),
                                  ((2, 64, 2), None), ((2, 72, 2), None), ((2, 78, 2), [73, 78]), ((1, 78, 2), None), ((1, 70, 2), None)]
    assert len(stub.prefills) == 1 and stub.closed


def test_token_limit_flushes_and_warns_once_per_row():
    with pytest.warns(RuntimeWarning) as rec:
        events, trace, stub, full = run([3, 40, None, None], 64)
    assert sorted(str(w.message).split("utterance ")[1][0] for w in rec if "max_mel_tokens" in str(w.message)) == ["2", "3"]
    assert trace["frames"][0] == [(0, 3)] and trace["frames"][1] == [(0, 5), (5, 40)]
    assert trace["frames"][2] == trace["frames"][3] == [(0, 5), (5, 13), (13, 21), (21, 64)]
    for b, T in enumerate([3, 40, 64, 64]):
        mine = [(pcm, last) for row, pcm, last in events if row == b]
        assert [last for _, last in mine] == [False] * (len(mine) - 1) + [True]
        assert torch.equal(torch.cat([p for p, _ in mine]), full[b, :T].float().repeat_interleave(HOP))


def test_empty_last_where_nothing_is_left():
    """No halo towards the future: a row that stops ON a boundary has emitted everything when its stop token is seen."""
    events, trace, stub, full = run([16, 20], 32, halo=(0, 0))
    assert trace["frames"] == [[(0, 8), (8, 16)], [(0, 8), (8, 16), (16, 20)]]
    mine = [(int(pcm.numel()), last) for row, pcm, last in events if row == 0]
    assert mine == [(8 * HOP, False), (8 * HOP, False), (0, True)]
    assert [(int(pcm.numel()), last) for row, pcm, last in events if row == 1] == [(8 * HOP, False), (8 * HOP, False), (4 * HOP, True)]
    assert [row for row, _, _ in events] == [0, 1, 0, 1, 0, 1]


def test_plan_of_one_boundary():
    from indextts.infer import IndexTTS
    codes = torch.tensor([[5, 6, STOP, STOP], [5, 6, 7, 8], [STOP] * 4, [1, 2, 3, 4]])
    plan = IndexTTS.stream_batch_plan(codes, [0, 0, 0, 1], [False, False, False, True], 1, 10, STOP)
    assert plan == [(0, 2, 0, 2, True), (1, 4, 0, 3, False), (2, 0, 0, 0, True)]         # row 3 has ended: not planned again
    assert IndexTTS.stream_batch_plan(codes[:, :1], [0] * 4, [False] * 4, 1, 10, STOP) == [(2, 0, 0, 0, True)]
    plan = IndexTTS.stream_batch_plan(codes, [2, 3, 0, 0], [False] * 4, 1, 4, STOP)       # n == max_mel_tokens: every row is final
    assert plan == [(0, 2, 2, 2, True), (1, 4, 3, 4, True), (2, 0, 0, 0, True), (3, 4, 0, 4, True)]


def test_the_batch_plan_is_the_one_planner_over_equivalent_records():
    """stream_batch_plan holds no rule of its own: over every n, limit, halo, stop position and drawn (ended, emitted) it returns what
    stream_queue_plan returns for the records of the rows that have not ended (k = n, not stopped) -- and both return what the rule
    stream_batch_plan held before it became that adapter returns (written out below)."""
    from indextts.infer import IndexTTS

    def rule(codes, emitted, ended, right, limit):
        n, out = int(codes.shape[1]), []
        for b in range(int(codes.shape[0])):
            if ended[b]:
                continue
            hit = (codes[b] == STOP).nonzero()
            final = bool(hit.numel()) or n >= limit
            k = int(hit[0]) if hit.numel() else n
            t1 = k if final else max(emitted[b], k - right)
            if t1 > emitted[b] or final:
                out.append((b, k, emitted[b], t1, final))
        return out
    rng, B, cases, finals = torch.Generator().manual_seed(5), 3, 0, 0
    for n in range(1, 13):
        for limit in (12, 16):
            for right in (0, 3):
                for pos in [None] + list(range(n)):
                    codes = torch.randint(0, 8000, (B, n), generator=rng)
                    if pos is not None:
                        codes[int(torch.randint(0, B, (1,), generator=rng)), pos] = STOP
                    ended = (torch.rand(B, generator=rng) < 0.3).tolist()
                    emitted = torch.randint(0, n + 1, (B,), generator=rng).tolist()
                    got = IndexTTS.stream_batch_plan(codes, emitted, ended, right, limit, STOP)
                    live = [b for b in range(B) if not ended[b]]
                    want = IndexTTS.stream_queue_plan([dict(utt=b, k=n, codes=codes[b], stopped=False) for b in live],
                                                      {b: emitted[b] for b in live}, right, limit, STOP)
                    assert got == want == rule(codes, emitted, ended, right, limit), (n, limit, right, pos, ended, emitted)
                    cases, finals = cases + 1, finals + sum(f for *_, f in got)
    assert cases == 12 * 2 * 2 + 2 * 2 * sum(range(1, 13)) and 0 < finals < 3 * cases


def stream_one(ends, limit, **kw):
    """stream_utterance itself over the stub: (chunks, trace, stub, full)."""
    from indextts.infer import IndexTTS
    polls, full = recorded_polls(ends, limit)
    stub, trace = StubTTS(polls), {}
    stub._stream_rows = types.MethodType(IndexTTS._stream_rows, stub)        # stream_utterance is its one-row form
    chunks = list(IndexTTS.stream_utterance(stub, None, torch.arange(3, dtype=torch.int32), chunk_tokens=CHUNK, max_mel_tokens=limit,
                                            seed=7, _trace=trace, **kw, **GEN))
    return chunks, trace, stub, full


@pytest.mark.parametrize("end,limit,frames", [(75, 96, [(0, 5), (5, 13), (13, 21), (21, 29), (29, 37), (37, 75)]),
                                              (None, 64, [(0, 5), (5, 13), (13, 21), (21, 64)])], ids=["stop-token", "token-limit"])
def test_one_utterance_is_the_batch_of_one_row_unwrapped(end, limit, frames):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        chunks, trace, stub, full = stream_one([end], limit)
    T = limit if end is None else end
    assert all(type(c) is torch.Tensor and c.dim() == 1 and c.numel() > 0 for c in chunks)      # pcm only, and no empty flush
    assert len(chunks) == len(frames) and torch.equal(torch.cat(chunks), full[0, :T].float().repeat_interleave(HOP))
    assert trace["frames"] == frames                              # flat: the lists of row 2 in the two tests above
    assert torch.equal(trace["codes"], full[0, :T]) and torch.equal(torch.cat(trace["latent"])[:, 0], full[0, :T].float())
    assert stub.latent_calls and all(rows == [0] for rows, _ in stub.latent_calls)
    assert [n for _, (n,) in stub.latent_calls] == [min(t1 + 35, T) for _, t1 in frames[:-1]] + [T]
    assert len(stub.vocoder_calls) == len(frames) and all(shape[0] == 1 and lens is None for shape, lens in stub.vocoder_calls)
    said = [str(w.message) for w in rec if "max_mel_tokens" in str(w.message)]
    assert len(said) == (end is None) and not any("utterance 0" in s for s in said)
    assert len(stub.prefills) == 1 and stub.closed


def test_an_early_close_abandons_the_loop():
    events, trace, stub, _ = run([3, 40, 75, 88], 96, stop_after=2)
    assert len(events) == 2 and stub.closed and len(stub.latent_calls) == 2


def test_refusals_come_before_anything_is_launched():
    from indextts.infer import IndexTTS
    nobody = types.SimpleNamespace()                 # no model, no device: the checks need neither
    rows = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
    with pytest.raises(NotImplementedError, match="beam"):
        IndexTTS.stream_batch(nobody, None, rows, num_beams=3)
    with pytest.raises(ValueError, match="one of them"):
        IndexTTS.stream_batch(nobody, None, rows, adapter_ids=[0, 1], adapter_mix=[{0: 0.5}, None])
    with pytest.raises(ValueError, match="adapter_ids"):
        IndexTTS.stream_batch(nobody, None, rows, adapter_ids=[0])
    with pytest.raises(ValueError, match="adapter_mix"):
        IndexTTS.stream_batch(nobody, None, rows, adapter_mix=[{0: 0.5}] * 3)
    with pytest.raises(ValueError, match="sampling"):
        IndexTTS.stream_batch(nobody, None, rows, sampling=[{"seed": 1}])
    with pytest.raises(ValueError, match="sampling"):
        IndexTTS.stream_batch(nobody, None, rows, sampling={"seed": 1})
    with pytest.raises(ValueError, match="unknown keys"):
        IndexTTS.stream_batch(nobody, None, rows, sampling=[{"seed": 1}, {"beams": 2}])
    with pytest.raises(ValueError, match="chunk_tokens"):
        IndexTTS.stream_batch(nobody, None, rows, chunk_tokens=0)
    with pytest.raises(ValueError, match="force_stop"):
        IndexTTS.stream_batch(nobody, None, rows, force_stop=[3])
    with pytest.raises(ValueError, match="prompts"):
        IndexTTS.stream_batch(nobody, [torch.zeros(1, 100, 9)], rows)
    with pytest.raises(TypeError, match="unknown generation settings"):
        IndexTTS.stream_batch(nobody, None, rows, beams=1)
    assert list(IndexTTS.stream_batch(nobody, None, [])) == []


class StubSentences:
    """infer_stream's surroundings: five sentences of one token each; stream_batch emits its rows interleaved."""

    def __init__(self):
        self.batches, self.alone = [], 0
        self.tokenizer = types.SimpleNamespace(tokenize=lambda text: text.split(), split_sentences=lambda toks, limit: [[t] for t in toks],
                                               convert_tokens_to_ids=lambda sent: [int(t) for t in sent])
        self.sent = {}

    def _prompt(self, path):
        return "mel of " + path

    def chunk(self, sentence, i):
        return self.sent.setdefault((sentence, i), torch.full((2,), 10.0 * sentence + i))

    def stream_utterance(self, cond_mel, ids, **kw):
        self.alone += 1
        for i in range(2):
            yield self.chunk(int(ids[0]), i)

    def stream_batch(self, cond_mel, rows, **kw):
        assert cond_mel == "mel of p.wav"
        self.batches.append(([int(r[0]) for r in rows], kw))
        s = [int(r[0]) for r in rows]
        empty = torch.zeros(0)
        if len(rows) == 3:       # the last row first; row 1 ends before row 0; row 2 ends with an empty flush
            plan = [(2, 0, False), (0, 0, False), (1, 0, False), (1, 1, True), (2, 1, False), (0, 1, True), (2, None, True)]
        else:                    # row 1 is over before row 0 says anything
            plan = [(1, 0, False), (1, 1, True), (0, 0, False), (0, 1, True)]
        for row, i, last in plan:
            yield row, (empty if i is None else self.chunk(s[row], i)), last


def test_parallel_sentences_come_out_in_text_order():
    from indextts.infer import IndexTTS
    stub = StubSentences()
    got = list(IndexTTS.infer_stream(stub, "p.wav", "0 1 2 3 4", parallel_sentences=3, chunk_tokens=4, seed=9, force_stop=[12]))
    assert stub.alone == 0 and [b for b, _ in stub.batches] == [[0, 1, 2], [3, 4]]
    assert stub.batches[0][1] == dict(chunk_tokens=4, seed=9, force_stop=[12, 12, 12]) and stub.batches[1][1]["force_stop"] == [12, 12]
    assert all(sr == 24000 for sr, _ in got)
    want = [stub.sent[(s, i)] for s in range(5) for i in range(2)]
    assert len(got) == len(want) == 10 and all(a is b for (_, a), b in zip(got, want))    # text order, nothing lost, no copies
    # sentence 0's chunks leave as they come: its first is out before row 1 has ended
    stub = StubSentences()
    it = IndexTTS.infer_stream(stub, "p.wav", "0 1 2", parallel_sentences=3)
    assert next(it)[1] is stub.sent[(0, 0)] and (1, 1) not in stub.sent
    it.close()


def test_one_sentence_at_a_time_never_enters_the_batch():
    from indextts.infer import IndexTTS
    stub = StubSentences()
    got = list(IndexTTS.infer_stream(stub, "p.wav", "0 1 2"))
    assert stub.alone == 3 and stub.batches == [] and len(got) == 6
    assert all(a is stub.sent[(s, i)] for (_, a), (s, i) in zip(got, [(s, i) for s in range(3) for i in range(2)]))
    with pytest.raises(ValueError):
        list(IndexTTS.infer_stream(stub, "p.wav", "0 1 2", parallel_sentences=0))
