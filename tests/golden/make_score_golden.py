#!/usr/bin/env python3
"""Generates tests/golden/score_small.npz: the reference's UnifiedVoice (2 layers, the name-hashed synthetic weights of tests/synth.py)
run on the CPU in this container (never on the GPU box) WITHOUT return_latent, for the likelihood-scoring tests
(tests/test_score_*.py).

Inputs: the three texts of make_golden.gpt_inputs(), 9 seeded random codes a row, wav_lengths = [9 * 1024, 5 * 1024 - 100, 2 * 1024]
(so that set_mel_padding matters).  The class runs once in fp32 and once in .double().  Written: the inputs, loss_text and loss_mel of
forward (both precisions), and per position and head, from the float64 logits: targets, t, lse, nll, rank, best, the best's margin
over the runner-up and near_m = the number of j with |l(j) - t| <= m for m in NEAR; the text logits come from get_logits with
text_head, as forward calls it.  max |logit32 - logit64| is recorded too, and the float64 final-norm rows of all three
utterances (the operands of both heads, [3, L + 2, D] and [3, T + 2, D]).  The codes come from numpy's default_rng(20261021).  Only data is written; no weights (synth regenerates them)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (installs the reference harness)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

NEAR = (1e-3, 2e-3, 4e-3)
N_CODES = 9
WAV_LENGTHS = [9 * 1024, 5 * 1024 - 100, 2 * 1024]


def logits_of(m, cond_mel, cml, text, text_lengths, codes, wav_lengths):
    """forward's own steps (model.py:561-591) up to get_logits: (text_logits [B, Vt, L + 2], mel_logits [B, Vm, T + 2], targets)."""
    conds = m.get_conditioning(cond_mel, cml)
    mel_len = torch.ceil(wav_lengths / m.mel_length_compression).long() + 1
    mel = m.set_mel_padding(codes.clone(), mel_len)
    txt = m.set_text_padding(text.clone(), text_lengths)
    txt = F.pad(txt, (0, 1), value=m.stop_text_token)
    mel = F.pad(mel, (0, 1), value=m.stop_mel_token)
    txt, txt_t = m.build_aligned_inputs_and_targets(txt, m.start_text_token, m.stop_text_token)
    mel, mel_t = m.build_aligned_inputs_and_targets(mel, m.start_mel_token, m.stop_mel_token)
    te = m.text_embedding(txt) + m.text_pos_embedding(txt)
    me = m.mel_embedding(mel) + m.mel_pos_embedding(mel)
    c = conds.expand(text.shape[0], -1, -1)
    tl, ml = m.get_logits(c, te, m.text_head, me, m.mel_head)
    return tl, ml, txt_t, mel_t, m.get_logits(c, te, m.text_head, me, m.mel_head, return_latent=True)


def per_position(logits, targets):
    """logits [B, V, N] float64, targets [B, N] -> dict of [B, N] arrays."""
    l = logits.permute(0, 2, 1)
    V = l.shape[-1]
    y = targets.long()
    t = l.gather(2, y[..., None])[..., 0]
    lse = torch.logsumexp(l, dim=2)
    j = torch.arange(V)[None, None]
    ahead = ((l > t[..., None]) | ((l == t[..., None]) & (j < y[..., None]))) & (j != y[..., None])
    top2 = torch.topk(l, 2, dim=2)
    out = dict(targets=y, t=t, lse=lse, nll=lse - t, rank=ahead.sum(2), best=l.argmax(2), margin=top2.values[..., 0] - top2.values[..., 1])
    for i, mm in enumerate(NEAR):
        out[f"near{i}"] = ((l - t[..., None]).abs() <= mm).sum(2)
    return {k: v.numpy() for k, v in out.items()}


def main():
    m = MG.build_gpt(2)
    cond_mel_np, _, text_np, lens = MG.gpt_inputs()
    rng = np.random.default_rng(20261021)
    codes_np = rng.integers(0, 8192, size=(3, N_CODES)).astype(np.int64)
    cond_mel, text, codes = torch.from_numpy(cond_mel_np), torch.from_numpy(text_np), torch.from_numpy(codes_np)
    cml = torch.tensor([cond_mel.shape[-1]])
    tlen, wl = torch.tensor(lens), torch.tensor(WAV_LENGTHS)
    out = dict(text=text_np, text_lens=np.array(lens), codes=codes_np, wav_lengths=np.array(WAV_LENGTHS), near=np.array(NEAR))
    res = {}
    for tag in ("32", "64"):
        mm, cm = (m, cond_mel) if tag == "32" else (m.double(), cond_mel.double())          # (.double() converts in place: fp32 first)
        lt, lm, _ = mm(cm.expand(3, -1, -1), text.clone(), tlen, codes.clone(), wl, cond_mel_lengths=cml.expand(3))
        out[f"loss_text_{tag}"], out[f"loss_mel_{tag}"] = float(lt), float(lm)
        res[tag] = logits_of(mm, cm, cml, text, tlen, codes, wl)
        print(f"fp{tag}: loss_text {float(lt):.6f} loss_mel {float(lm):.6f}")
    tl, ml, tt, mt, lat = res["64"]
    # the heads' operands in float64, every position of every utterance, for the CPU statement test
    out["text_lat64"], out["mel_lat64"] = lat[0].numpy(), lat[1].numpy()
    out["logit_err_32"] = max((res["32"][0].double() - tl).abs().max().item(), (res["32"][1].double() - ml).abs().max().item())
    for name, lg, tg in (("text", tl, tt), ("mel", ml, mt)):
        for k, v in per_position(lg, tg).items():
            out[f"{name}_{k}"] = v
        ce = F.cross_entropy(lg, tg.long()).item()
        assert abs(ce - out[f"loss_{name}_64"]) < 1e-9, (name, ce, out[f"loss_{name}_64"])
    path = os.path.join(HERE, "score_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes); max |logit32 - logit64| {out['logit_err_32']:.2e}; mel logits {tuple(ml.shape)}")


if __name__ == "__main__":
    main()
