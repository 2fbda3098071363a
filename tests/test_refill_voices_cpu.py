"""Continuous batching with voices on the host side (no GPU): the join's entry point is declared, exported and bound; a fed item names
its voice as a fourth element and the 2- and 3-tuples mean what they meant; infer_queue checks its voice arguments before anything
is launched, carries every utterance's voice into the loop that serves it -- leftovers included -- and into its latent pass."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_exports_and_binds_the_join():
    from indextts import _native as nat
    L = nat.lib()
    assert L.itts_abi_version() == 10
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "indextts_hip.h")).read(), flags=re.S)
    assert "itts_refill_join" in re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", txt) and "itts_refill_join" in nat.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), "itts_refill_join") and callable(nat.refill_join)
    # the struct as the header lays it out (LP64), field by field in the header's order
    fields = re.search(r"typedef struct itts_refill_join_args \{(.*?)\} itts_refill_join_args;", txt, re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in nat.RefillJoinArgs._fields_]
    assert ctypes.sizeof(nat.RefillJoinArgs) == 232 and nat.RefillJoinArgs.s_l.offset == 48 and nat.RefillJoinArgs.i_b.offset == 88
    assert nat.RefillJoinArgs.rows.offset == 112 and nat.RefillJoinArgs.step0.offset == 160 and nat.RefillJoinArgs.state.offset == 224
    a = nat.RefillJoinArgs()
    assert L.itts_refill_join(ctypes.byref(a), None) == 1 and b"itts_refill_join" in L.itts_last_error()
    with pytest.raises(nat.NativeError):             # the wrapper wants device tensors: there is no host path
        z = torch.zeros(2, dtype=torch.int32)
        nat.refill_join(torch.zeros(2, 1, 1, 64), torch.zeros(2, 1, 1, 64), torch.zeros(1, 2, 1, 4, 64), torch.zeros(1, 2, 1, 4, 64), z, z, z,
                        z, z, z, z, 0, z, torch.zeros(2, 8, dtype=torch.int32), z, z, z, z, torch.zeros(8, dtype=torch.int32))


def bare_engine(n):
    from indextts.gpt.engine import GPTEngine
    eng = object.__new__(GPTEngine)
    eng.bank = None if n is None else SimpleNamespace(n=n, rp=16, Kx=64, sig=(n, 16, ()))
    return eng


def test_a_fed_item_names_its_voice_as_a_fourth_element():
    from indextts.gpt.engine import GPTEngine
    p = torch.zeros(3, 64)
    sp = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=3, stream=0)
    items = [(p, 5), (p, 5, None), (p, 5, sp), (p, 5, None, 2), (p, 5, sp, {0: .7, 1: .3}), (p, 5, None, None), (p, 5, None, -1),
             (p, 5, None, [(1, .5)])]
    assert [GPTEngine._fed_voice(it) for it in items] == [None, None, None, 2, {0: .7, 1: .3}, None, -1, [(1, .5)]]
    eng = bare_engine(3)
    assert eng.check_adapter_mix([GPTEngine._fed_voice(it) for it in items], 8) == \
        [(), (), (), ((2, 1.0),), ((0, .7), (1, .3)), (), (), ((1, .5),)]
    # the 2- and 3-tuples keep their meaning: the pair is the pair, the third element the row's settings or the loop's default
    assert all(tuple(it)[:2] == (p, 5) for it in items)
    default = dict(sp, seed=9)
    assert GPTEngine._fed_settings(items[0], default) == default and GPTEngine._fed_settings(items[1], default) == default
    assert GPTEngine._fed_settings(items[2], default)["seed"] == 3 and GPTEngine._fed_settings(items[4], default)["seed"] == 3
    assert GPTEngine._fed_settings(items[3], default) == default
    with pytest.raises(ValueError):
        GPTEngine._fed_settings(items[3], None)
    for bad in (3, {0: .2, 1: .2, 2: .2, 3: .2, 4: .2}, [(0, 1.0), 1]):        # id >= n, five entries, the id and pair forms at once
        with pytest.raises(ValueError):
            eng.check_adapter_mix([GPTEngine._fed_voice((p, 5, None, bad))], 1)


def test_decode_refill_refuses_on_the_host():
    """Nothing of the engine's device state exists on these bare engines: every refusal comes before any of it is touched."""
    feed = lambda k: []   # noqa: E731
    with pytest.raises(NotImplementedError, match="voices="):
        bare_engine(3).decode_refill(4, {}, feed)
    with pytest.raises(ValueError, match="no adapter bank"):
        bare_engine(None).decode_refill(4, {}, feed, voices=[0])
    with pytest.raises(ValueError, match="join"):
        bare_engine(3).decode_refill(4, {}, feed, voices=[0], join="index_put")
    eng = bare_engine(3)
    eng._B, eng._S, eng._shared_prefix, eng._kv_rows = 2, 40, None, None
    with pytest.raises(ValueError, match="holds 3 mixes"):
        eng.decode_refill(4, {}, feed, voices=[0, 1, 2])
    with pytest.raises(ValueError, match=r"ids must lie in \[0, 3\)"):
        eng.decode_refill(4, {}, feed, voices=[0, 3])
    eng._mix_host, eng._ids_host = None, [0, 2]
    with pytest.raises(ValueError, match="prefilled under"):
        eng.decode_refill(4, {}, feed, voices=[0, 1])
    eng._shared_prefix = (2, 3)
    with pytest.raises(ValueError, match="num_beams = 1"):
        eng.decode_refill(4, {}, feed, voices=[0, 2])


class _NoLaunchEngine:
    def __init__(self, bank):
        self.bank = bank

    def __getattr__(self, name):
        if name in ("_voices", "_row_adapters", "check_adapter_mix"):      # the host-side checks themselves
            from indextts.gpt.engine import GPTEngine
            return getattr(GPTEngine, name).__get__(self)
        raise AssertionError(f"engine.{name} was reached: the arguments are checked before anything is launched")


def _stub_tts(engine):
    from indextts.infer import IndexTTS
    tts = IndexTTS.__new__(IndexTTS)
    tts._gpt = SimpleNamespace(engine=engine)
    return tts


def test_infer_queue_checks_its_voices_before_any_launch():
    a = torch.zeros(1, 100, 40)
    texts = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
    bank = SimpleNamespace(n=3, rp=16, Kx=64, sig=())
    tts = _stub_tts(_NoLaunchEngine(bank))
    with pytest.raises(NotImplementedError, match=r"adapter_ids=\[-1\] \* N"):
        tts.infer_queue(a, texts, num_beams=1)
    with pytest.raises(ValueError, match="mutually exclusive"):
        tts.infer_queue(a, texts, num_beams=1, adapter_ids=[0, 1], adapter_mix=[0, 1])
    with pytest.raises(ValueError, match="holds 3 ids"):
        tts.infer_queue(a, texts, num_beams=1, adapter_ids=[0, 1, 2])
    with pytest.raises(ValueError, match="must lie in"):
        tts.infer_queue(a, texts, num_beams=1, adapter_ids=[0, 3])
    with pytest.raises(ValueError, match="at most 4 entries"):
        tts.infer_queue(a, texts, num_beams=1, adapter_mix=[0, {0: .2, 1: .2, 2: .2, 3: .2, 4: .2}])
    with pytest.raises(NotImplementedError, match="num_beams = 1"):
        tts.infer_queue(a, texts, adapter_ids=[0, 1])                        # the default is the reference's num_beams = 3
    plain = _stub_tts(_NoLaunchEngine(None))
    for kw in (dict(adapter_ids=[0, 1]), dict(adapter_mix=[0, None]), dict(adapter_ids=[-1, -1])):
        with pytest.raises(ValueError, match="no adapter bank"):
            plain.infer_queue(a, texts, num_beams=1, **kw)


@pytest.mark.parametrize("form", ["adapter_ids", "adapter_mix"])
def test_infer_queue_carries_every_voice_into_its_loop_and_its_latent_pass(form):
    """A stub engine that hands the last fed utterance back as leftover once: it re-enters the next loop under its own voice, and
    every group of the closing latent pass is called with its utterances' voices."""
    from indextts.gpt.engine import GPTEngine
    N, D = 5, 8
    given = [0, 2, -1, 1, 2] if form == "adapter_ids" else [0, {0: .7, 1: .3}, None, {2: 1.2}, 1]
    eng = bare_engine(3)
    eng.paged, eng.kv, eng._S = True, object(), 0
    want = GPTEngine._voices(eng, given, None, N)[0] if form == "adapter_ids" else eng.check_adapter_mix(given, N)
    log = SimpleNamespace(prefills=[], loops=[], latents=[])

    def prefill(emb, pad, max_new, **kw):
        log.prefills.append(kw)

    def decode_refill(max_new, sp, feed, voices=None, **kw):
        first = log.prefills[-1][form]
        assert list(voices) == list(first)
        fed = [it for _ in range(3) for it in feed(1)]
        assert all(len(it) == 4 and it[2] is None for it in fed)
        back = [fed.pop()] if len(log.loops) == 0 and fed else []
        log.loops.append((list(first), [it[3] for it in fed], [it[3] for it in back]))
        return [torch.tensor([7, 7, 8193])] * (len(first) + len(fed)), back
    eng.prefill, eng.decode_refill = prefill, decode_refill
    tts = _stub_tts(eng)
    tts.gpt.prefix_rows = lambda conds, bh: (torch.zeros(bh.shape[0], bh.shape[1] + 2, D), torch.zeros(bh.shape[0], dtype=torch.int32))
    tts.cfg = SimpleNamespace(gpt=SimpleNamespace(stop_text_token=1))
    tts._check_prompts = lambda cond_mel, n, gen, who: cond_mel
    tts._prompt_features = lambda cond_mel: (torch.zeros(1, 2, D), torch.zeros(1, 4))
    tts.remove_long_silence = lambda c: (c, torch.tensor([c.shape[1]]))
    tts._latents = lambda conds, texts, codes, **kw: log.latents.append((texts, kw)) or [torch.zeros(3, D)] * len(texts)
    tts._vocode_ragged = lambda lat, spk: [torch.zeros(4)] * len(lat)
    texts = [torch.arange(2, 2 + n) for n in (9, 8, 7, 6, 5)]                 # longest first: the queue's order is the input order
    outs = tts.infer_queue(torch.zeros(1, 100, 40), texts, slots=2, num_beams=1, **{form: given})
    assert len(outs) == N
    (f1, fed1, back1), (f2, fed2, back2) = log.loops
    assert f1 == want[0:2] and fed1 == want[2:4] and back1 == [want[4]]       # utterance 4 was fed and handed back ...
    assert f2 == [want[4]] and fed2 == [] and back2 == []                     # ... and starts the next loop under its own voice
    assert all(form in kw and not {"adapter_ids", "adapter_mix"} - {form} & set(kw) for kw in log.prefills)
    seen = {}
    for group, kw in log.latents:
        assert set(kw) == {form} and len(kw[form]) == len(group)
        for t, v in zip(group, kw[form]):
            seen[int(t.numel())] = v
    assert [seen[n] for n in (9, 8, 7, 6, 5)] == want
