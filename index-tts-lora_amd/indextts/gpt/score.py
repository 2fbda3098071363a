"""Likelihood scoring: how likely are GIVEN tokens under the decoder's output heads?

head_scores_torch is the readable statement of the quantities, in plain torch on any device; ScoreEngine computes them on the device
with libindextts_score.so (include/indextts_score.h) -- one target-logit launch and one streamed pass per head, the [rows][vocabulary]
logits never stored.  UnifiedVoice.score and IndexTTS.score_codes are built on it.  Nothing here is imported by a default path.
"""
from __future__ import annotations

import torch

from .. import _native_score as nl
from ..utils import quant


def head_scores_torch(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, y: torch.Tensor) -> dict:
    """The quantities of include/indextts_score.h from materialised logits: x [R, D], W [D, >= V] (columns past V = len(b) are not
    looked at), b [V], y [R] integer targets; a target outside [0, V) marks an ignored row (nll 0, t 0, rank -1).  Everything is
    computed in x's dtype.  -> dict of t, lse, nll [R] (x's dtype) and rank, best [R] (int64)."""
    V = b.numel()
    logits = x @ W[:, :V].to(x.dtype) + b.to(x.dtype)
    y = y.to(logits.device).long()
    real = (y >= 0) & (y < V)
    ys = torch.where(real, y, torch.zeros_like(y))
    t = logits.gather(1, ys[:, None])[:, 0]
    lse = torch.logsumexp(logits, dim=1)
    j = torch.arange(V, device=logits.device)[None]
    ahead = (logits > t[:, None]) | ((logits == t[:, None]) & (j < ys[:, None]))
    rank = (ahead & (j != ys[:, None])).sum(1)
    # the first column holding the maximum: the smallest j among equals
    best = (logits == logits.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
    zero = torch.zeros_like(t)
    return dict(t=torch.where(real, t, zero), lse=lse, nll=torch.where(real, lse - t, zero),
                rank=torch.where(real, rank, torch.full_like(rank, -1)), best=best)


class ScoreEngine:
    """The two output heads of a GPTEngine's checkpoint as libindextts_score.so takes them, and the launches over them.

    Keeps row-major copies W [D][ldw] of mel_head and text_head (ldw = V rounded up to a multiple of 8, the pad columns zero) in
    the engine's dtype and the biases in fp32.  An FP8 engine (weight_dtype "fp8") scores with the values its own passes see: the
    16-bit rounding of its DEQUANTISED mel head; text_head, which the engine never loads, is taken in 16 bits.  Owns the workspace;
    score() is one ittl_target_logit + one ittl_head_nll for any number of rows."""

    def __init__(self, engine, state_dict):
        self.device, self.dtype = engine.device, engine.dtype
        self.heads = {}
        for name in ("mel", "text"):
            wk, bk = f"{name}_head.weight", f"{name}_head.bias"
            if wk not in state_dict or bk not in state_dict:
                raise RuntimeError(f"ScoreEngine: the checkpoint holds no {wk} / {bk}")
            w = state_dict[wk].detach().to(self.device, torch.float64).t()            # [D, V]
            if name == "mel" and engine.weight_dtype == "fp8":
                w = quant.dequantize(*quant.quantize_e4m3_cols(w))
            D, V = w.shape
            W = torch.zeros(D, nl.pitch(V), dtype=self.dtype, device=self.device)
            W[:, :V] = w.to(torch.float32).to(self.dtype)
            self.heads[name] = (W, state_dict[bk].detach().to(self.device, torch.float32).contiguous())
        self._ws = None

    def score(self, x: torch.Tensor, y: torch.Tensor, head: str = "mel") -> dict:
        """x fp32 [R, D] (final-norm rows, as GPTEngine.latent returns them), y [R] integer targets (outside [0, V): ignored) ->
        dict of nll, lse, t (fp32 [R]) and rank, best (int32 [R]) on the device."""
        W, b = self.heads[head]
        x = x.to(self.device, torch.float32).contiguous()
        R, V = x.shape[0], b.numel()
        yl = y.to(self.device).reshape(-1).long()
        yi = torch.where((yl >= 0) & (yl < V), yl, torch.full_like(yl, -1)).to(torch.int32)   # (an int64 id must not wrap into range)
        need = nl.ws_bytes(R, V)
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        f = torch.empty(3, R, dtype=torch.float32, device=self.device)
        i = torch.empty(2, R, dtype=torch.int32, device=self.device)
        nl.target_logit(x, W, b, yi, f[0])
        nl.head_nll(x, W, b, yi, f[0], f[1], f[2], i[0], i[1], ws=self._ws if need else None)
        return dict(t=f[0], nll=f[1], lse=f[2], best=i[0], rank=i[1])


def aligned_targets(tokens: torch.Tensor, lengths: torch.Tensor, stop: int) -> torch.Tensor:
    """The reference's targets for `tokens` [B, N] of which row b holds lengths[b] real ones: positions past the length become
    `stop` (set_text_padding / set_mel_padding), one stop is appended (forward) and build_aligned_inputs_and_targets appends
    another: [B, N + 2].  The INPUT of position p is the start token for p = 0 and target p - 1 after it."""
    ar = torch.arange(tokens.shape[1], device=tokens.device)[None]
    padded = torch.where(ar < lengths.reshape(-1, 1), tokens, torch.full_like(tokens, stop))
    return torch.nn.functional.pad(padded, (0, 2), value=stop)
