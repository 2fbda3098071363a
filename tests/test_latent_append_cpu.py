"""The incremental latent pass, the parts that need no GPU: the C ABI is unchanged with the new wrapper present, the wrapper's
and the cache's refusals come before anything is launched, and -- over the stub engines of tests/test_stream_batch_cpu.py and
tests/test_stream_queue_cpu.py -- the three streams with latent_cache=True send every prompt row and every mel row of an
utterance through GPTEngine.latent_append exactly ONCE, reset a finished utterance's cache row before its next owner's first
rows, and yield the events of latent_cache=False."""
import types

import pytest
import torch

import test_stream_batch_cpu as sb
import test_stream_queue_cpu as sq

NC = 2           # conditioning rows of the stubs' prompts
START_MEL = 8192


# ---------------------------------------------------------------------------------------------------------------- ABI, wrapper
def test_the_abi_is_unchanged_and_the_wrapper_is_there():
    from indextts import _native
    assert callable(_native.attn_prefill_append)
    assert len(_native.EXPORTED_SYMBOLS) == 47 and "itts_attn_prefill_shared" in _native.EXPORTED_SYMBOLS
    assert _native.lib().itts_abi_version() == 10


def test_the_wrapper_refuses_before_any_launch():
    from indextts import _native as nat
    H, smax = 2, 64
    qkv, out = torch.zeros(4, 3 * 128), torch.zeros(4, 128)
    kc, vc = torch.zeros(1, H, smax, 64), torch.zeros(1, H, smax, 64)
    i = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    tail = (i(0, 4), i(0), i(0), i(0), 1)

    def call(kc=kc, vc=vc, w_row=tail[2], w_pos0=tail[3], Smax=4, qkv=qkv, **kw):
        nat.attn_prefill_append(qkv, out, kc, vc, tail[0], tail[1], w_row, w_pos0, 1, Smax, H, smax, **kw)
    with pytest.raises(nat.NativeError, match="kv_tab"):
        call(kv_tab=i(*[0] * 64), kv_bs=16)
    for missing in (dict(kc=None), dict(vc=None), dict(w_row=None), dict(w_pos0=None)):
        with pytest.raises(nat.NativeError, match="required"):
            call(**missing)
    with pytest.raises(nat.NativeError, match="contiguous"):
        call(kc=torch.zeros(1, H, smax, 128)[..., :64])
    with pytest.raises(nat.NativeError, match="one dtype"):
        call(kc=kc.to(torch.bfloat16), vc=vc.to(torch.bfloat16))
    with pytest.raises(nat.NativeError, match="one dtype"):
        call(qkv=qkv.to(torch.float16))
    with pytest.raises(nat.NativeError, match=r"\[rows\]"):
        call(kc=torch.zeros(1, H, 32, 64), vc=torch.zeros(1, H, 32, 64))
    with pytest.raises(nat.NativeError, match="Smax"):
        call(Smax=0)
    with pytest.raises(nat.NativeError, match="device tensors"):     # all of the above came first: host tensors never reach a launch
        call()


def test_the_c_side_refuses_the_same_without_a_launch():
    """The entry point itself, with pointers that are never dereferenced on the host: a paged table and missing caches."""
    import ctypes as C
    from indextts import _native as nat
    L, P = nat.lib(), C.c_void_p(64)
    assert L.itts_attn_prefill_shared(P, P, P, P, P, P, None, P, P, 1, 8, 2, 64, 0, P, 16, None) != 0
    assert "paged" in L.itts_last_error().decode()
    assert L.itts_attn_prefill_shared(P, P, None, None, P, P, None, P, P, 1, 8, 2, 64, 0, None, 0, None) != 0
    assert "null pointer" in L.itts_last_error().decode()
    assert L.itts_attn_prefill_shared(P, P, P, P, P, P, None, P, P, 1, 0, 2, 64, 0, None, 0, None) != 0
    assert "bad shape" in L.itts_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- the cache
def fake_engine(L=24, D=1280, H=20, dtype=torch.bfloat16):
    from indextts.gpt.engine import GPTEngine
    ns = types.SimpleNamespace(L=L, D=D, H=H, dtype=dtype, device="cpu", LATENT_CACHE_BUDGET=GPTEngine.LATENT_CACHE_BUDGET)
    ns.latent_cache = types.MethodType(GPTEngine.latent_cache, ns)
    return ns


def test_cache_sizing_budget_and_reset():
    from indextts.gpt.engine import GPTEngine, LatentCache
    assert LatentCache.nbytes(24, 1280, 1, 1024, torch.bfloat16) == 24 * 2 * 1280 * 1024 * 2 == 125829120      # "126 MB per row"
    assert GPTEngine.LATENT_CACHE_BUDGET == 8 << 30
    big = fake_engine()
    with pytest.raises(ValueError, match="budget"):         # 69 rows of 1 024 positions: 8.7 GB -- refused before torch allocates
        big.latent_cache(69, 1000)
    with pytest.raises(ValueError, match="at least 1"):
        big.latent_cache(0, 64)
    c = fake_engine(L=2, D=128, H=2, dtype=torch.float32).latent_cache(3, 65)
    assert c.cap == 128 and c.rows == 3 and c.kc.shape == c.vc.shape == (2, 3, 2, 128, 64) and c.kc.dtype == torch.float32
    assert not c.kc.any() and not c.vc.any() and c.have.tolist() == [0, 0, 0] and c.voice == [None] * 3
    c.have[1], c.voice[1] = 40, ("id", 2)
    c.kc[:, 1, :, :40] = 1.0
    c.reset(1)
    assert c.have.tolist() == [0, 0, 0] and c.voice[1] is None and bool(c.kc[:, 1, :, :40].all())     # nothing is cleared


# ---------------------------------------------------------------------------------------------------------------- row accounting
class Appends:
    """GPTEngine.latent_cache / latent_append and the embedding tables on the host: a table row holds (token, position, 0), so
    the stub reads from the rows it is given which utterance they belong to (name(cache row, first text token)) and which mel
    positions they are; the latent of mel position p is 1000 * name + p, the value of code p in the stubs -- what their _latents
    returns for that frame.  log: ("append", cache row, prompt rows, first mel position, mel rows) and ("reset", cache row)."""

    def __init__(self, eng, name):
        self.log, self.name, self.names, self.mel_have, self.cap = [], name, {}, {}, None
        tab = lambda n: torch.stack([torch.arange(n).float(), torch.zeros(n), torch.zeros(n)], 1)      # noqa: E731
        pos = lambda n: torch.stack([torch.zeros(n), torch.arange(n).float(), torch.zeros(n)], 1)      # noqa: E731
        eng.text_emb, eng.text_pos, eng.mel_emb, eng.mel_pos = tab(16000), pos(64), tab(16000), pos(256)
        eng.latent_cache, eng.latent_append = self.latent_cache, self.latent_append

    def latent_cache(self, rows, cap):
        from indextts.gpt.engine import LatentCache
        c = LatentCache(1, 1, rows, (cap + 63) // 64 * 64, torch.float32, "cpu")
        real = c.reset
        c.reset = lambda row: (self.log.append(("reset", int(row))), real(row))[1]
        self.cap = c.cap
        return c

    def latent_append(self, cache, emb, n_lens, cache_rows, adapter_ids=None, adapter_mix=None):
        assert len(set(cache_rows)) == len(cache_rows) == len(n_lens) and emb.shape[0] == sum(n_lens)
        out, o = torch.zeros_like(emb), 0
        for r, n in zip(cache_rows, n_lens):
            rows, prompt = emb[o: o + n], 0
            if cache.have[r] == 0:                          # cond | start_text text stop_text | start codes ...
                prompt = NC + self.text_len(rows)
                self.names[r], self.mel_have[r] = self.name(r, int(rows[NC + 1, 0])), 0
                assert int(rows[prompt, 0]) == START_MEL
            p = rows[prompt:, 1].long()
            assert p.tolist() == list(range(self.mel_have[r], self.mel_have[r] + len(p))), "mel positions continue where the row stands"
            out[o + prompt: o + n, 0] = 1000.0 * self.names[r] + p
            self.log.append(("append", int(r), prompt, int(p[0]), len(p)))
            cache.have[r] += n
            self.mel_have[r] += len(p)
            assert cache.have[r] <= cache.cap
            o += n
        return out

    @staticmethod
    def text_len(rows):
        """start_text (token 0) | text | stop_text (token 1) behind the NC conditioning rows: the number of text rows"""
        toks = rows[NC:, 0].long().tolist()
        assert toks[0] == 0
        return toks.index(1, 1) + 1


def tokens(stub):
    stub.gpt.start_text_token, stub.gpt.stop_text_token, stub.gpt.start_mel_token = 0, 1, START_MEL


def bind(stub, name):
    from indextts.infer import IndexTTS
    tokens(stub)
    app = Appends(stub.gpt.engine, name)
    stub._latents_incremental = types.MethodType(IndexTTS._latents_incremental, stub)
    return app


def per_utterance(log):
    """the log cut at the resets: per cache row, the utterances it served as (prompt rows, mel rows, [(first pos, count)])"""
    served, cur = [], {}
    for ev in log:
        if ev[0] == "reset":
            if ev[1] in cur:
                served.append((ev[1], cur.pop(ev[1])))
        else:
            _, r, prompt, p0, n = ev
            u = cur.setdefault(r, dict(prompt=0, mel=0, spans=[], prompts=0))
            assert p0 == u["mel"], "a mel row was skipped or sent twice"
            u["prompt"], u["mel"], u["prompts"] = u["prompt"] + prompt, u["mel"] + n, u["prompts"] + (prompt > 0)
            assert (prompt > 0) == (len(u["spans"]) == 0), "the prompt goes with a row's first rows only"
            u["spans"].append((p0, n))
    return served + list(cur.items())


def same_events(a, b):
    assert [(u, last) for u, _, last in a] == [(u, last) for u, _, last in b]
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))


def test_stream_batch_sends_every_row_once():
    from indextts.infer import IndexTTS
    ends, limit = [44, 90, 61], 96
    off, _, _, _ = sb.run(ends, limit)
    polls, _ = sb.recorded_polls(ends, limit)
    stub, trace = sb.StubTTS(polls), {}
    stub._prompt_features = lambda cond_mel: (torch.zeros(1, NC, 3), torch.zeros(1, 1, 4))
    app = bind(stub, lambda row, first: row)
    texts = [torch.arange(3 + b, dtype=torch.int32) + 2 for b in range(3)]
    on = list(IndexTTS._stream_rows(stub, None, texts, sb.CHUNK, limit, 7, None, None, None, None, trace, dict(sb.GEN), True))
    same_events(on, off)
    assert not stub.latent_calls                              # the repeated pass never ran
    served = dict(per_utterance(app.log))
    for b, T in enumerate(ends):
        assert served[b]["prompt"] == NC + (3 + b) + 2 and served[b]["prompts"] == 1
        assert served[b]["mel"] == T                          # start | codes[:T-1]: T rows for T frames, each once
    assert sum(n for ev in app.log if ev[0] == "append" for n in (ev[2] + ev[4],)) == sum(NC + 3 + b + 2 + T for b, T in enumerate(ends))
    assert app.cap >= 3 + limit + 2                           # (the stub's prefix is 3 rows long)


def test_stream_utterance_sends_every_row_once():
    from indextts.infer import IndexTTS
    polls, _ = sb.recorded_polls([70], 96)

    def make():
        stub = sb.StubTTS(polls)
        stub._prompt_features = lambda cond_mel: (torch.zeros(1, NC, 3), torch.zeros(1, 1, 4))
        stub._latents = lambda conds, texts, codes, **kw: [c.float()[:, None].expand(-1, 3) for c in codes]
        stub._stream_rows = types.MethodType(IndexTTS._stream_rows, stub)        # stream_utterance is its one-row form
        return stub
    text = torch.tensor([5, 6, 7], dtype=torch.int32)
    kw = dict(chunk_tokens=sb.CHUNK, max_mel_tokens=96, seed=7, force_stop=[70], **sb.GEN)
    off = list(IndexTTS.stream_utterance(make(), None, text, **kw))
    stub = make()
    app = bind(stub, lambda row, first: 0)
    on = list(IndexTTS.stream_utterance(stub, None, text, latent_cache=True, **kw))
    assert len(on) == len(off) > 3 and all(torch.equal(a, b) for a, b in zip(on, off))
    (row, u), = per_utterance(app.log)
    assert row == 0 and u["prompt"] == NC + 3 + 2 and u["mel"] == 70 and len(u["spans"]) > 3
    assert all(n <= sb.CHUNK for _, n in u["spans"][1:])     # a boundary costs its new rows, not all k


def test_stream_queue_sends_every_row_once_and_resets_a_slot_before_its_next_owner():
    from indextts.infer import IndexTTS
    names, ends = [(10, 12), (11, 5), (12, 17), (13, 9), (14, 14)], [44, 60, 38, 75, 52]
    off, t_off, _ = sq.run(names, ends)
    stub = sq.StubQueueTTS()
    app = bind(stub, lambda row, first: first)
    reqs = [dict(handle=i, text=sq.text_of(nm, ln), prompt=0, stop=e, sp=None, voice=None) for i, ((nm, ln), e) in enumerate(zip(names, ends))]
    trace = {}
    on = list(IndexTTS._stream_queue(stub, "mel", reqs, 2, sq.CHUNK, 96, 7, None, None, trace, dict(sq.GEN), None, True))
    same_events(on, off)
    sq.check_contract(on, trace, [nm for nm, _ in names], ends)
    assert not stub.latent_calls
    served = per_utterance(app.log)
    assert len(served) == 5 and {row for row, _ in served} == {0, 1}           # five utterances through two cache rows
    by_name = {}
    for row, u in served:
        assert u["prompts"] == 1
        by_name[(u["prompt"], u["mel"])] = row
    assert sorted(by_name) == sorted((NC + ln + 2, e) for (_, ln), e in zip(names, ends))
    total = sum(ev[2] + ev[4] for ev in app.log if ev[0] == "append")
    assert total == sum(NC + ln + 2 + e for (_, ln), e in zip(names, ends))   # prompt + codes, not the quadratic count
    # a slot's reset lies between its two owners: in the log, every "append with a prompt" on a row that has served before
    # is preceded by that row's reset
    dirty = set()
    for ev in app.log:
        if ev[0] == "reset":
            dirty.discard(ev[1])
        else:
            assert not (ev[2] > 0 and ev[1] in dirty), f"cache row {ev[1]} was handed on without a reset"
            dirty.add(ev[1])
    assert app.cap >= NC + 17 + 2 + 96 + 2                   # sized for the queue's longest prompt + max_mel_tokens + 2


def test_stream_queue_resets_a_row_once_between_two_owners_and_every_row_at_a_new_loop():
    """Where the resets lie, over a fake incremental pass that records (cache row, utterance, codes) and a fake cache that records
    its resets, each with the number of the loop it happened in.  Two slots, four utterances: 10 (2 codes) and 11 (20 codes) start;
    17 arrives, takes slot 0 from 10 inside the first loop and stops with 11 at the poll n = 25; 16, whose prompt is longer than
    the positions that loop has passed, is held back and starts a second loop alone."""
    from indextts.gpt.model import row_sampling_params
    from indextts.infer import IndexTTS
    stub, log = sq.StubQueueTTS(), []
    stub.gpt.engine.latent_cache = lambda rows, cap: types.SimpleNamespace(reset=lambda row: log.append(("reset", stub.loops, int(row))))

    def incremental(st, rows, conds, text_rows, code_rows, **kw):
        log.extend(("rows", stub.loops, int(r), int(t[0])) for r, t in zip(rows, text_rows))
        return [c.float()[:, None].expand(-1, 2) for c in code_rows]
    stub._latents_incremental = incremental
    held = dict(handle="held", text=sq.text_of(16, 38), force_stop=40)
    late = dict(handle="late", text=sq.text_of(17, 4), force_stop=5)
    more, _ = sq.scripted_more([[held, late]])
    sp = row_sampling_params([{}] * 2, 2, sq.GEN, 7)
    reqs = [dict(handle=i, text=sq.text_of(nm, 5), prompt=0, stop=e, sp=sp[i], voice=None) for i, (nm, e) in enumerate([(10, 2), (11, 20)])]
    events = list(IndexTTS._stream_queue(stub, "mel", reqs, 2, sq.CHUNK, 96, 7, None, more, {}, dict(sq.GEN), None, True))
    assert stub.loops == 2 and not stub.latent_calls and sorted(str(h) for h, _, last in events if last) == ["0", "1", "held", "late"]
    served = [ev[1:] for ev in log if ev[0] == "rows"]
    assert served == [(1, 0, 10), (1, 0, 17), (1, 1, 11), (2, 0, 16)]         # (loop, cache row = slot, utterance)
    owner, resets = {}, {}                                  # per cache row: (loop, utterance) it last served; resets since then
    for kind, loop, row, *name in log:
        if kind == "reset":
            resets[row] = resets.get(row, 0) + 1
            continue
        before = owner.get(row)
        if before is not None and before != (loop, name[0]):
            assert resets[row] >= 1, f"cache row {row} was handed on without a reset"
            if before[0] == loop:
                assert resets[row] == 1, f"cache row {row}: {resets[row]} resets between two owners of one loop"
        owner[row], resets[row] = (loop, name[0]), 0
    # the second loop has prefilled every slot anew: both rows are reset in it, before its first rows are sent
    first = log.index(("rows", 2, 0, 16))
    assert {ev[2] for ev in log[:first] if ev[:2] == ("reset", 2)} == {0, 1}


def test_a_request_too_long_for_the_cache_is_refused_like_any_other():
    stub = sq.StubQueueTTS(max_text_tokens=8)
    bind(stub, lambda row, first: first)
    script = iter([[dict(handle="late", text=sq.text_of(15, 30))], None])
    refused, trace = [], {}
    from indextts.infer import IndexTTS
    reqs = [dict(handle=0, text=sq.text_of(10, 6), prompt=0, stop=20, sp=None, voice=None)]
    from indextts.gpt.model import row_sampling_params
    reqs[0]["sp"] = row_sampling_params([{}], 1, sq.GEN, 7)[0]
    events = list(IndexTTS._stream_queue(stub, "mel", reqs, 2, sq.CHUNK, 96, 7, None, lambda: next(script), trace, dict(sq.GEN), refused, True))
    assert [h for h, e in refused] == ["late"] and "latent cache" in str(refused[0][1])
    assert {u for u, _, _ in events} == {0}
