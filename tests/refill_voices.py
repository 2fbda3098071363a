"""Shared pieces of the tests of continuous batching with voices (decode_refill(voices=...), infer_queue(adapter_ids= / adapter_mix=)):
the 2-layer full-width model, a 3-adapter bank and the merged checkpoints as tests/test_lora_mix_engine_gpu.py builds them (copied,
that file stays as it is), a queue runner over GPTEngine.decode_refill and a teacher-forced one-row run that returns logits."""
import numpy as np
import torch

import synth
import weights

DEV = "cuda"
TARGETS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
GREEDY = dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=10.0, seed=0)


def make_factors(sd, ranks, scalings, layers=2, seed=3):
    """[(adapters, scaling)] on all four targets of every layer: the bank in the attach_lora_bank format."""
    g = torch.Generator().manual_seed(seed)
    bank = []
    for r, sc in zip(ranks, scalings):
        ad = {}
        for i in range(layers):
            for name in TARGETS:
                key = f"gpt.h.{i}.{name}"
                k_in, n_out = sd[key + ".weight"].shape
                ad[key] = (torch.randn(r, k_in, generator=g) * 0.02, torch.randn(n_out, r, generator=g) * 0.02)
        bank.append((ad, sc))
    return bank


def merged_state(sd, bank, mix):
    """The checkpoint with the mix merged: W + sum_j w_j s_j A_j^T B_j^T in fp32 (mix: {id: weight} or None)."""
    ms = dict(sd)
    for a, w in (mix or {}).items():
        ad, sc = bank[a]
        for key, (A, Bm) in ad.items():
            ms[key + ".weight"] = ms[key + ".weight"].float() + (A.t() @ Bm.t()) * (sc * w)
    return ms


def make_model(state, dtype):
    from indextts.gpt.model import UnifiedVoice
    m = UnifiedVoice(**dict(weights.reference_config()["gpt"], layers=2))
    m.load_state_dict(state)
    m.to(DEV).to(dtype).post_init_gpt2_config(kv_cache=True)
    return m


def as_mix(voice):
    """{id: weight} of a voice given as None / -1 / id / dict."""
    if voice is None or voice == -1:
        return None
    return dict(voice) if isinstance(voice, dict) else {int(voice): 1.0}


class Voices:
    """One checkpoint, a bank of three adapters (ranks 4 / 8 / 16), one prompt and texts of mixed lengths, longest first."""
    LENS = [14, 12, 11, 9, 8, 7, 6, 5]

    def __init__(self):
        self.sd = weights.gpt_state_dict(2)
        self.bank = make_factors(self.sd, (4, 8, 16), (2.0, 1.0, 0.5))
        self.cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
        rng = np.random.default_rng(21)
        self.texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in self.LENS]
        self._models = {}

    def model(self, dtype, bank=True):
        k = (dtype, bank)
        if k not in self._models:
            m = make_model(self.sd, dtype)
            self._models[k] = m.attach_lora_bank(self.bank) if bank else m
        return self._models[k]

    def merged(self, voice, dtype=torch.float32):
        return make_model(merged_state(self.sd, self.bank, as_mix(voice)), dtype)

    def prefix(self, m, texts):
        L = max(int(t.numel()) for t in texts)
        bh = torch.full((len(texts), L), m.stop_text_token, dtype=torch.int32)
        for j, t in enumerate(texts):
            bh[j, : t.numel()] = t
        return m.prefix_rows(m.get_conditioning(self.cond_mel, None), bh)

    def queue(self, m, order, stops, slots, voices=None, sp=GREEDY, settings=None, texts=None, max_new=40, check_every=4, trace=None,
              **kw):
        """The utterances `order` (indices into texts / stops / voices / settings) through `slots` decode slots: the first `slots`
        are prefilled, the others fed in order.  Returns {utterance: codes on the host}.  trace (a list): receives (n, slots) of
        every join, in order."""
        eng, texts = m.engine, self.texts if texts is None else texts
        first, rest = list(order[:slots]), list(order[slots:])
        emb, pad = self.prefix(m, [texts[i] for i in first])
        eng.prefill(emb, pad, 400, **({} if voices is None else {"adapter_mix": [voices[i] for i in first]}))
        fed = []

        def feed(k):
            take = [rest.pop(0) for _ in range(min(k, len(rest)))]
            if not take:
                return []
            fed.extend(take)
            e, p = self.prefix(m, [texts[i] for i in take])
            p = p.tolist()
            tail = lambda i: () if voices is None and settings is None else (None if settings is None else settings[i],) + \
                (() if voices is None else (voices[i],))   # noqa: E731
            return [(e[j, p[j]:], stops[i]) + tail(i) for j, i in enumerate(take)]

        join = eng._join
        if trace is not None:
            def traced(st, *a, **k2):
                trace.append((st["n"], list(st["rows_h"]), st["logits"].clone()))
                return join(st, *a, **k2)
            eng._join = traced
        try:
            codes, leftover = eng.decode_refill(max_new, sp if settings is None else [settings[i] for i in first], feed,
                                                force_stop=[stops[i] for i in first], check_every=check_every,
                                                **({} if voices is None else {"voices": [voices[i] for i in first]}), **kw)
        finally:
            if trace is not None:
                del eng._join
        assert not leftover and len(codes) == len(order) and eng.refill_stats["rows_refilled"] == len(order) - slots
        return {i: c.cpu() for i, c in zip(first + fed, codes)}

    def alone(self, m, i, stop, voice, max_new=40, bank=True):
        """(codes [n], logits [n, V]) of utterance i prefilled and decoded alone, greedy, under `voice`."""
        kw = dict(adapter_mix=[voice]) if bank else {}
        c, lg = m.inference_speech(self.cond_mel, self.texts[i][None].to(DEV), do_sample=False, num_beams=1, repetition_penalty=10.0,
                                   max_generate_length=max_new, force_stop=[stop], return_logits=True, **kw)
        return c[0].cpu(), lg[:, 0].cpu()

    def forced_logits(self, m, text, codes, voice=None):
        """Logits [len(codes), V] of one row run alone and teacher-forced with `codes`: entry s is the distribution token s was
        drawn from.  voice: the row's voice on a model with a bank (None on a merged / plain model)."""
        eng = m.engine
        emb, pad = self.prefix(m, [text])
        n = int(codes.numel())
        out = [eng.prefill(emb, pad, n + 2, **({} if eng.bank is None else {"adapter_mix": [voice]}))[:1].clone()]
        eng.force_stop[:1] = -1
        skip, eng.skip_finished = eng.skip_finished, False
        try:
            for s in range(1, n):
                eng._sample(1, GREEDY)
                eng.tokens[:1] = int(codes[s - 1])
                eng.history[:1, s - 1] = int(codes[s - 1])
                eng.finished[:1] = 0
                eng._step_transformer(1)
                out.append(eng.logits[:1].clone())
        finally:
            eng.skip_finished = skip
        return torch.cat(out, 0).float().cpu()


def same_up_to_a_tie(c, want, lg, tag):
    """The rule of test_decode_refill_gives_every_row_the_codes_it_gets_alone: codes equal those of the stand-alone run up to the
    first step whose top-2 margin in the stand-alone logits is below 1e-3 (another left padding, another reduction order)."""
    for s_ in range(c.numel()):
        if int(c[s_]) != int(want[s_]):
            top2 = torch.topk(lg[s_], 2).values
            assert (top2[0] - top2[1]).item() < 1e-3, (tag, s_, c, want)
            break
