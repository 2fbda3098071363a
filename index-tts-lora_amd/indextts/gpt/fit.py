"""Voice fitting: train the reference's LoRA (train.py:548-605, finetune_models/config.yaml) on a frozen
GPTEngine and hand back (adapters, scaling) in the attach_lora format.

Where the work runs.  The blocks' GEMMs, forward and backward, frozen and low-rank alike, are the project's plain GEMM
(nat.gemm_conv, split-K in slices of 256 reduction elements where its form applies: _mm): y = x W + b, then u = drop(x) A^T and y += s u B^T as two small products; backward dx = dy W^T over a transposed
packed copy of W made once per fit, du = s dy B, dx += (du A) . mask.  The two factor gradients dB^T = s u^T dy and dA = du^T drop(x)
are ittf_lora_wgrad, the squared gradient norm ittf_sqnorm and the LoRA+ AdamW update ittf_adamw_step (libindextts_fit.so,
include/indextts_fit.h).  LayerNorm, GELU, the causal attention, the two heads and their cross-entropy run as torch ops on the
device and autograd carries their backward: plumbing, named as follow-up kernels in DESIGN -- but under FitConfig(attention="hip")
the attention, forward and backward, is ittf_attn_fwd / ittf_attn_bwd (_Attn).  Nothing here is imported by a default
path, and nothing of the engine changes: the fit reads the engine's packed weights and writes only tensors of its own.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

TARGETS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
_WKEY = {"attn.c_attn": "w_qkv", "attn.c_proj": "w_o", "mlp.c_fc": "w_fc", "mlp.c_proj": "w_pr"}
_BKEY = {"attn.c_attn": "b_qkv", "attn.c_proj": "b_o", "mlp.c_fc": "b_fc", "mlp.c_proj": "b_pr"}
MAX_RANK = 64      # the voice pool's own limit (ITTF_MAX_RANK)
ATTENTIONS = ("torch", "hip")


@dataclass
class FitConfig:
    """The reference's finetune_models/config.yaml (train.lora, train.optimizer, train) as defaults."""
    rank: int = 4
    alpha: float = 8.0
    targets: tuple = TARGETS
    dropout: float = 0.2
    text_weight: float = 0.1
    lr: float = 5.0e-6
    loraplus_lr_ratio: float = 2.0
    weight_decay: float = 0.01
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    max_grad_norm: float | None = 1.0
    total_steps: int = 100            # optimizer steps the cosine schedule spans
    warmup_ratio: float = 0.1
    seed: int = 0
    start_text_token: int = 0
    stop_text_token: int = 1
    mel_length_compression: int = 1024
    attention: str = "torch"          # "hip": ittf_attn_fwd / ittf_attn_bwd in the place of the per-utterance torch loop (section 4.30)

    def check(self):
        """Every refusal of a configuration, before anything is launched."""
        if self.attention not in ATTENTIONS:
            raise ValueError(f"fit: attention must be one of {ATTENTIONS} (got {self.attention!r})")
        if not isinstance(self.rank, int) or not 1 <= self.rank <= MAX_RANK:
            raise ValueError(f"fit: rank must be an integer in [1, {MAX_RANK}] (got {self.rank!r})")
        targets = tuple(self.targets)
        bad = [t for t in targets if t not in TARGETS]
        if bad or not targets or len(set(targets)) != len(targets):
            raise ValueError(f"fit: targets must be a non-empty subset of {TARGETS} (got {targets})")
        if not 0.0 <= float(self.dropout) < 1.0:
            raise ValueError(f"fit: dropout must lie in [0, 1) (got {self.dropout})")
        if not 0.0 <= float(self.text_weight) <= 1.0:
            raise ValueError(f"fit: text_weight must lie in [0, 1] (got {self.text_weight})")
        if not (float(self.lr) > 0 and float(self.loraplus_lr_ratio) > 0 and float(self.weight_decay) >= 0 and float(self.alpha) > 0):
            raise ValueError("fit: lr, loraplus_lr_ratio and alpha must be positive, weight_decay not negative")
        if int(self.total_steps) < 1 or not 0.0 <= float(self.warmup_ratio) <= 1.0:
            raise ValueError("fit: total_steps must be at least 1 and warmup_ratio lie in [0, 1]")
        if self.max_grad_norm is not None and not float(self.max_grad_norm) > 0:
            raise ValueError("fit: max_grad_norm must be positive (or None: no clipping)")
        return self


def cosine_with_warmup(step: int, warmup: int, total: int) -> float:
    """The factor of transformers.get_cosine_schedule_with_warmup (num_cycles 0.5) for the optimizer step about to be taken
    (0-based: the number of steps taken so far)."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    progress = float(step - warmup) / float(max(1, total - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))


def init_factors(K: int, N: int, r: int, gen: torch.Generator):
    """peft's LoRA initialisation: A [r, K] kaiming-uniform with a = sqrt(5) -- uniform in +- 1 / sqrt(K) -- and B zero.  B is
    returned transposed, B^T [r, N]: the layout of its gradient u^T dy."""
    bound = 1.0 / math.sqrt(K)
    A = (torch.rand(r, K, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
    return A, torch.zeros(r, N, dtype=torch.float32)


def check_engine(engine, who="fit_voice"):
    """What a fit cannot run on, by message (as attach_lora refuses it)."""
    if engine.weight_dtype is not None:
        raise ValueError(f"{who}(): fitting on an FP8 base is not built (weight_dtype='fp8'): the frozen GEMMs, forward and backward, "
                         "take 16-bit or fp32 packed weights")
    if engine.kv_dtype is not None:
        raise NotImplementedError(f"{who}(): fitting on an engine with the FP8 KV cache (kv_dtype='fp8') is not built: the voice it "
                                  "produced could not be attached to it")
    if engine.lora:
        raise ValueError(f"{who}(): single adapters are attached (attach_lora(None) first): the fit trains on the base weights")


def check_rows(text_rows, code_rows, batch_rows: int | None, n_cond: int = 0, who="fit_voice"):
    """The host checks of a training set: list lengths, empty rows, and batch_rows against the longest utterance (cond | start text
    stop | start codes stop stop).  -> the row count of every utterance."""
    if len(text_rows) != len(code_rows):
        raise ValueError(f"{who}: {len(code_rows)} code rows for {len(text_rows)} texts")
    if not len(text_rows):
        raise ValueError(f"{who}: no utterance")
    rows = []
    for i, (t, c) in enumerate(zip(text_rows, code_rows)):
        if int(t.numel()) < 1 or int(c.numel()) < 1:
            raise ValueError(f"{who}: utterance {i} has no text tokens or no codes")
        rows.append(n_cond + int(t.numel()) + 2 + int(c.numel()) + 2)
    if batch_rows is not None and max(rows) > int(batch_rows):
        raise ValueError(f"{who}: batch_rows = {batch_rows} is too small for the longest utterance ({max(rows)} rows)")
    return rows


def plan_batches(rows, batch_rows: int):
    """Utterance indices in batches, in order, each padded batch (utterances x its longest) within batch_rows rows."""
    out, cur, longest = [], [], 0
    for i, n in enumerate(rows):
        if cur and max(longest, n) * (len(cur) + 1) > batch_rows:
            out.append(cur)
            cur, longest = [], 0
        cur.append(i)
        longest = max(longest, n)
    if cur:
        out.append(cur)
    return out


class _Target:
    """One adapted GEMM of one block: the engine's packed W [K, N] and bias, the transposed packed copy for dx, and -- when the target
    is trained -- the fp32 masters A [r, K], B^T [r, N], their gradients and moments, the T copies [rp, .] the GEMMs read (rows >= r
    zero) and the four packed operands made from them."""
    adapted = False


K_SLICE = 256     # reduction elements of one split-K slice of a fit GEMM (below)


def _mm(T, x, wp, K, N):
    """x [M, K] (T) times the packed W [K, N] -> fp32 [M, N] through nat.gemm_conv.  A gradient is a small difference of long sums,
    and Adam's first updates divide it by its own magnitude, so the fit's reductions are kept short: where the kernel's split-K
    form applies (N a multiple of 128) K is cut into slices of K_SLICE, each summed by the matrix pipe on its own, and the slices'
    fp32 slabs are added in rising order (itts_rows) -- a chain of K_SLICE / 4 (fp32) steps and K / K_SLICE additions in the place of one chain
    of K / 4.  Measured on the 3-step trajectory test."""
    from .. import _native as nat
    M = x.shape[0]
    ks = K // K_SLICE if N % 128 == 0 and K % K_SLICE == 0 else 1
    if ks < 2:
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        nat.gemm_conv(T, 1, M, M, K, N, wp, x, y, y_f32=True)
        return y
    slab = torch.empty(ks, M, N, dtype=torch.float32, device=x.device)
    nat.gemm_conv(T, 1, M, M, K, N, wp, x, slab, y_f32=True, ksplit=ks)
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    nat.rows(M * (N // 128), 128, T, slab=slab, nslab=ks, y=y)     # one launch: the slabs in rising order (elementwise: any row width)
    return y


class _Gemm(torch.autograd.Function):
    """y = x W + b + s (drop(x) A^T) B^T over fp32 rows x [M, K] -> fp32 [M, N]; the operands are rounded to the engine's dtype, every
    product is nat.gemm_conv with fp32 accumulation (_mm).  `hook` is a scalar that requires grad: it makes autograd call backward
    for a GEMM whose input does not (the first block's), and its own gradient is None."""

    @staticmethod
    def forward(ctx, x, hook, fe, tg, mask):
        from .. import _native as nat
        T = fe.dtype
        M, K, N = x.shape[0], tg.K, tg.N
        xT = x.detach().to(T).contiguous()
        y = _mm(T, xT, tg.w, K, N).add_(tg.bias)
        xd = u = None
        if tg.adapted:
            xd = xT if mask is None else (x.detach() * mask).to(T).contiguous()
            u = _mm(T, xd, tg.at_pack, K, fe.rp).to(T)
            nat.gemm_conv(T, 1, M, M, fe.rp, N, tg.bt_pack, u, y, y_f32=True, accumulate=True, scale=fe.scaling)
        ctx.fe, ctx.tg, ctx.mask = fe, tg, mask
        ctx.save_for_backward(xT, xd if xd is not xT else None, u)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .. import _native as nat
        from .. import _native_fit as nf
        fe, tg, mask = ctx.fe, ctx.tg, ctx.mask
        xT, xd, u = ctx.saved_tensors
        xd = xT if xd is None else xd
        T = fe.dtype
        M, K, N = xT.shape[0], tg.K, tg.N
        dyT = dy.to(T).contiguous()
        dx = _mm(T, dyT, tg.wt, N, K)
        if tg.adapted:
            r, acc = fe.cfg.rank, fe._accumulate
            du = _mm(T, dyT, tg.b_pack, N, fe.rp).mul_(fe.scaling).to(T)                    # du = s dy B
            ws = fe._workspace(nf.wgrad_ws_bytes(M, r, max(K, N)))
            nf.lora_wgrad(u, dyT, tg.gBt, ws, r=r, accumulate=acc, scale=fe.scaling)        # dB^T = s u^T dy
            nf.lora_wgrad(du, xd, tg.gA, ws, r=r, accumulate=acc)                           # dA = du^T drop(x)
            if fe.probe is not None:     # (tests) M and sum_m |s z| of both reductions: what ittf_lora_wgrad's bound is made of
                mag = lambda a, b: a[:, :r].double().abs().t() @ b.double().abs()          # noqa: E731
                fe.probe.setdefault(tg.key, []).append((M, mag(du, xd), fe.scaling * mag(u, dyT)))
            if mask is None:
                nat.gemm_conv(T, 1, M, M, fe.rp, K, tg.a_pack, du, dx, y_f32=True, accumulate=True)
            else:
                t = torch.empty_like(dx)
                nat.gemm_conv(T, 1, M, M, fe.rp, K, tg.a_pack, du, t, y_f32=True)
                dx.addcmul_(t, mask)
        return dx, None, None, None, None


class _Attn(torch.autograd.Function):
    """FitConfig(attention="hip"): the causal attention of every utterance of a batch in one launch over the c_attn GEMM's fp32
    output qkv [M, 3 D], read in place -> fp32 [M, D], the row-major operand of attn.c_proj (ittf_attn_fwd).  Saved: qkv and
    lse [H, M]; the backward recomputes the probabilities and needs no out (ittf_attn_bwd).  Rows outside `rows` -- the rectangle's padding -- stay
    zero in out and in dqkv, as F.pad leaves them in the torch arm."""

    @staticmethod
    def forward(ctx, qkv, fe, rows):
        from .. import _native_fit as nf
        qkv = qkv.detach().contiguous()
        out, lse = nf.attn_fwd(qkv, rows, fe.H, 0.125)
        ctx.fe, ctx.rows = fe, rows
        ctx.save_for_backward(qkv, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _native_fit as nf
        qkv, lse = ctx.saved_tensors
        fe = ctx.fe
        ws = fe._attn_workspace(nf.attn_ws_bytes(ctx.rows.M, fe.H))
        return nf.attn_bwd(qkv, lse, dout.contiguous(), ctx.rows, fe.H, 0.125, ws=ws), None, None


class FitEngine:
    """The trainer of one voice over a GPTEngine and the checkpoint it was loaded from.  step(batch) is one optimizer step (a list
    of batches: gradient accumulation over them), evaluate(batch) the losses without dropout, voice() the trained (adapters,
    scaling), state_dict() / load_state_dict() the resume file (tensors and numbers only).

    A batch is either the padded form UnifiedVoice.score takes -- dict(conds [1 | B, C, D], text [B, L], text_lengths [B], codes
    [B, T], wav_lengths [B]), with that call's padding, alignment and means -- or the ragged form batch() builds from rows, in which
    every utterance is laid out as a batch of its own (what IndexTTS.score_codes scores, and what fit_voice trains on)."""

    def __init__(self, engine, state_dict, config: FitConfig | None = None):
        from .. import _native as nat
        from .. import _native_fit as nf
        self.cfg = cfg = (config or FitConfig()).check()
        check_engine(engine, "FitEngine")
        for k in ("text_head.weight", "text_head.bias", "mel_head.weight", "mel_head.bias"):
            if k not in state_dict:
                raise RuntimeError(f"FitEngine: the checkpoint holds no {k}")
        nf.lib()
        self.engine, self.device, self.dtype = engine, engine.device, engine.dtype
        dev, T = self.device, self.dtype
        self.L, self.D, self.H = engine.L, engine.D, engine.H
        self.scaling = float(cfg.alpha) / float(cfg.rank)
        self.rp = 128                                    # the small products' K / N, zero-padded: the width at which split-K applies
        self.step_count, self._accumulate, self._ws, self._attn_ws = 0, False, None, None
        self.probe = None          # a dict here collects, per target and backward, (M, sum |du x|, s sum |u dy|): see _Gemm.backward
        self._hook = torch.zeros((), dtype=torch.float32, device=dev, requires_grad=True)
        self.heads = {}
        for name in ("text", "mel"):
            w = state_dict[f"{name}_head.weight"].detach().to(dev, torch.float32)
            self.heads[name] = (w.to(T).to(torch.float32).contiguous(),                    # [V, D]: the ScoreEngine's rounded operand
                                state_dict[f"{name}_head.bias"].detach().to(dev, torch.float32).contiguous())
        gen = torch.Generator().manual_seed(int(cfg.seed))
        self.targets, entries = [], []
        for i, l in enumerate(engine.layers):
            row = {}
            for name in TARGETS:
                tg = _Target()
                key = f"gpt.h.{i}.{name}"
                W = engine._W[key + ".weight"].detach().to(dev, torch.float32)           # Conv1D: [K, N]
                tg.key, tg.K, tg.N = key, int(W.shape[0]), int(W.shape[1])
                tg.w, tg.bias = l[_WKEY[name]], l[_BKEY[name]]
                tg.wt = nat.pack_weight(W.t().to(T).contiguous())
                if name in cfg.targets:
                    tg.adapted = True
                    A, Bt = init_factors(tg.K, tg.N, cfg.rank, gen)
                    tg.A, tg.Bt = A.to(dev), Bt.to(dev)
                    for f in ("A", "Bt"):
                        p = getattr(tg, f)
                        setattr(tg, "g" + f, torch.zeros_like(p))
                        setattr(tg, "m" + f, torch.zeros_like(p))
                        setattr(tg, "v" + f, torch.zeros_like(p))
                        setattr(tg, f + "_T", torch.zeros(self.rp, p.shape[1], dtype=T, device=dev))
                    # the T copies' first r rows are one contiguous run: the segment's t_copy
                    entries.append((tg.A, tg.gA, tg.mA, tg.vA, tg.A_T[: cfg.rank], 0))
                    entries.append((tg.Bt, tg.gBt, tg.mBt, tg.vBt, tg.Bt_T[: cfg.rank], 1))
                row[name] = tg
            self.targets.append(row)
        self.table = nf.SegmentTable(entries, dev)
        self._refresh(copy=True)

    # ---------------------------------------------------------------------------------------------- factors
    def _adapted(self):
        return [tg for row in self.targets for tg in row.values() if tg.adapted]

    def _refresh(self, copy=False):
        """The packed operands of the small products from the T copies (ittf_adamw_step wrote them; copy=True: from the masters, at
        the start and after load_state_dict): A^T [K, rp] and A [rp, K], B^T [rp, N] and B [N, rp], through pack_weight."""
        from .. import _native as nat
        r = self.cfg.rank
        for tg in self._adapted():
            if copy:
                tg.A_T[:r].copy_(tg.A)
                tg.Bt_T[:r].copy_(tg.Bt)
            tg.a_pack, tg.at_pack = nat.pack_weight(tg.A_T), nat.pack_weight(tg.A_T.t().contiguous())
            tg.bt_pack, tg.b_pack = nat.pack_weight(tg.Bt_T), nat.pack_weight(tg.Bt_T.t().contiguous())

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _attn_workspace(self, nbytes):
        """ittf_attn_bwd's workspace (its own: a wgrad of the same backward must not grow it away)."""
        if self._attn_ws is None or self._attn_ws.numel() < nbytes:
            self._attn_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._attn_ws

    def voice(self):
        """(adapters, scaling) in the attach_lora format: {"gpt.h.{i}.{target}": (A [r, in], B [out, r])}, alpha / r."""
        return {tg.key: (tg.A.detach().clone(), tg.Bt.detach().t().contiguous()) for tg in self._adapted()}, self.scaling

    def grads(self):
        """{key: (dA [r, in], dB [out, r])} of the last backward (clones), in voice()'s layout."""
        return {tg.key: (tg.gA.clone(), tg.gBt.t().contiguous()) for tg in self._adapted()}

    def set_factors(self, adapters):
        """Overwrite the masters with `adapters` (voice()'s format, every trained target): tests and warm starts."""
        for tg in self._adapted():
            A, B = adapters[tg.key]
            if tuple(A.shape) != tuple(tg.A.shape) or tuple(B.shape) != (tg.N, self.cfg.rank):
                raise ValueError(f"set_factors: {tg.key}: A {tuple(A.shape)}, B {tuple(B.shape)} do not fit rank {self.cfg.rank}")
            tg.A.copy_(A.to(self.device, torch.float32))
            tg.Bt.copy_(B.to(self.device, torch.float32).t())
        self._refresh(copy=True)

    def state_dict(self):
        sd = {"step": int(self.step_count), "seed": int(self.cfg.seed), "rank": int(self.cfg.rank), "alpha": float(self.cfg.alpha)}
        for tg in self._adapted():
            for f in ("A", "Bt", "mA", "mBt", "vA", "vBt"):
                sd[f"{tg.key}.{f}"] = getattr(tg, f).detach().cpu().clone()
        return sd

    def load_state_dict(self, sd):
        if int(sd["rank"]) != self.cfg.rank or float(sd["alpha"]) != float(self.cfg.alpha) or int(sd["seed"]) != int(self.cfg.seed):
            raise ValueError("load_state_dict: the file was written under another rank, alpha or seed")
        for tg in self._adapted():
            for f in ("A", "Bt", "mA", "mBt", "vA", "vBt"):
                t = sd[f"{tg.key}.{f}"]
                if tuple(t.shape) != tuple(getattr(tg, f).shape):
                    raise ValueError(f"load_state_dict: {tg.key}.{f} has shape {tuple(t.shape)}")
                getattr(tg, f).copy_(t.to(self.device, torch.float32))
        self.step_count = int(sd["step"])
        self._refresh(copy=True)

    # ---------------------------------------------------------------------------------------------- batches
    def batch(self, conds, text_rows, code_rows):
        """Ragged rows -> a ragged batch: every utterance is its own sequence cond | start text stop | start codes stop stop, as
        UnifiedVoice.score lays out a batch of that utterance alone; the sequences are right-padded to the longest with zero rows
        that no real row sees (causal attention) and no loss counts.  The losses are the means over all utterances' positions."""
        B = len(text_rows)
        check_rows(text_rows, code_rows, None, who="FitEngine.batch")
        if conds.shape[0] not in (1, B):
            raise ValueError(f"FitEngine.batch: conds holds {conds.shape[0]} prompts for {B} utterances (one for all, or one per row)")
        return dict(conds=conds, text_rows=[t.reshape(-1).cpu().long() for t in text_rows],
                    code_rows=[c.reshape(-1).cpu().long() for c in code_rows])

    def _inputs(self, b):
        """-> emb [B, S, D] fp32 and per head (flat row indices into [B * S], flat targets, positions per utterance, real positions
        per utterance: its tokens and the first stop).  A padded batch (text, text_lengths, codes, wav_lengths) gets
        UnifiedVoice.score's padding and alignment (model.py:565-588); a ragged one (text_rows, code_rows) that of each utterance
        alone."""
        from .score import aligned_targets
        eng, dev, cfg = self.engine, self.device, self.cfg
        c = b["conds"].to(dev, torch.float32)
        nc = int(c.shape[1])
        if "text_rows" in b:
            B = len(b["text_rows"])
            one = lambda v: torch.tensor([v])                                            # noqa: E731
            tts = [aligned_targets(t[None], one(t.numel()), cfg.stop_text_token)[0] for t in b["text_rows"]]
            mts = [aligned_targets(m[None], one(m.numel()), eng.stop_mel)[0] for m in b["code_rows"]]
            S = max(nc + t.numel() + m.numel() for t, m in zip(tts, mts))
            emb = torch.zeros(B, S, self.D, dtype=torch.float32, device=dev)
            emb[:, :nc] = c if c.shape[0] == B else c[0]
            heads = {"text": [[], [], [], []], "mel": [[], [], [], []]}
            for i, (tt, mt) in enumerate(zip(tts, mts)):
                at = nc
                for name, tgt, start, table, pos in (("text", tt, cfg.start_text_token, eng.text_emb, eng.text_pos),
                                                     ("mel", mt, eng.start_mel, eng.mel_emb, eng.mel_pos)):
                    ids = F.pad(tgt[:-1], (1, 0), value=start).to(dev)
                    emb[i, at: at + ids.numel()] = table[ids] + pos[: ids.numel()]
                    h = heads[name]
                    h[0].append(i * S + at + torch.arange(ids.numel()))
                    h[1].append(tgt)
                    h[2].append(int(ids.numel()))
                    h[3].append(int(ids.numel()) - 1)
                    at += ids.numel()
            lens = [nc + t.numel() + m.numel() for t, m in zip(tts, mts)]
            return emb, {k: (torch.cat(h[0]).to(dev), torch.cat(h[1]).to(dev), h[2], h[3]) for k, h in heads.items()}, lens
        text = b["text"].to(dev).long()
        codes = b["codes"].to(dev).long()
        B = int(text.shape[0])
        tl = torch.as_tensor(b["text_lengths"]).to(dev).long().reshape(-1)
        wl = torch.as_tensor(b["wav_lengths"]).to(dev).reshape(-1)
        ml = torch.ceil(wl.float() / cfg.mel_length_compression).long() + 1
        tt = aligned_targets(text, tl, cfg.stop_text_token)
        mt = aligned_targets(codes, ml, eng.stop_mel)
        ti = F.pad(tt[:, :-1], (1, 0), value=cfg.start_text_token)
        mi = F.pad(mt[:, :-1], (1, 0), value=eng.start_mel)
        te = eng.text_emb[ti] + eng.text_pos[: ti.shape[1]]
        me = eng.mel_emb[mi] + eng.mel_pos[: mi.shape[1]]
        if c.shape[0] == 1 and B > 1:
            c = c.expand(B, -1, -1)
        emb = torch.cat([c, te, me], dim=1).contiguous()
        S, nt, nm = emb.shape[1], tt.shape[1], mt.shape[1]
        base = torch.arange(B, device=dev)[:, None] * S + nc
        rows_t = (base + torch.arange(nt, device=dev)[None]).reshape(-1)
        rows_m = (base + nt + torch.arange(nm, device=dev)[None]).reshape(-1)
        return emb, {"text": (rows_t, tt.reshape(-1), [nt] * B, [int(n) + 1 for n in tl.tolist()]),
                     "mel": (rows_m, mt.reshape(-1), [nm] * B, [int(n) for n in ml.tolist()])}, [S] * B    # (mel_len counts the first stop)

    # ---------------------------------------------------------------------------------------------- the pass
    def _attention(self, qkv, lens, S, causal, rows):
        """The causal attention of one block over the c_attn GEMM's output qkv [M, 3 D] -> [M, D], the rectangle's padding rows
        zero.  rows None: the torch loop; otherwise the row table of the batch (attention="hip"): one launch, _Attn."""
        if rows is not None:
            return _Attn.apply(qkv, self, rows)
        H, D = self.H, self.D
        qkv = qkv.view(len(lens), S, 3, H, 64)
        att = []
        for i, n in enumerate(lens):     # per utterance over its own rows: the same shapes -- the same bits -- alone and in any batch
            q, k, v = qkv[i, :n].permute(1, 2, 0, 3)                                       # each [H, n, 64]
            sc = (torch.matmul(q, k.transpose(-1, -2)) * 0.125).masked_fill(~causal[:n, :n], float("-inf"))
            a = torch.matmul(torch.softmax(sc, dim=-1), v).permute(1, 0, 2).reshape(n, D)
            att.append(F.pad(a, (0, 0, 0, S - n)))
        return torch.cat(att, 0)

    def _forward(self, b, train: bool, gen=None):
        emb, heads, lens = self._inputs(b)
        B, S, D = emb.shape
        H, M, p = self.H, B * S, float(self.cfg.dropout)
        dev = self.device
        h = emb.view(M, D)
        causal = torch.ones(S, S, dtype=torch.bool, device=dev).tril()
        rows = None
        if self.cfg.attention == "hip":      # the row table, once per batch: utterance i is rows i S .. i S + lens[i] - 1
            from .. import _native_fit as nf
            rows = nf.AttnRows([(i * S, n) for i, n in enumerate(lens)], M, dev)

        def gemm(x, tg):
            mask = None
            if train and p > 0 and tg.adapted:
                mask = (torch.rand(x.shape, generator=gen, device=dev) >= p).to(torch.float32) / (1.0 - p)
            return _Gemm.apply(x, self._hook, self, tg, mask)

        for l, tgs in zip(self.engine.layers, self.targets):
            xn = F.layer_norm(h, (D,), l["ln1"][0], l["ln1"][1], 1e-5)
            att = self._attention(gemm(xn, tgs["attn.c_attn"]), lens, S, causal, rows)
            h = h + gemm(att, tgs["attn.c_proj"])
            xn = F.layer_norm(h, (D,), l["ln2"][0], l["ln2"][1], 1e-5)
            ff = F.gelu(gemm(xn, tgs["mlp.c_fc"]), approximate="tanh")
            h = h + gemm(ff, tgs["mlp.c_proj"])
        eng = self.engine
        enc = F.layer_norm(F.layer_norm(h, (D,), eng.ln_f[0], eng.ln_f[1], 1e-5), (D,), eng.final_norm[0], eng.final_norm[1], 1e-5)
        enc = enc.view(M, D)
        out = {}
        for name, (rows, tgt, counts, real) in heads.items():
            W, bias = self.heads[name]
            x = enc[rows]
            if self.dtype != torch.float32:
                x = x.to(self.dtype).to(torch.float32)
            nll, at = [], 0
            for n in counts:                 # per utterance, for the same reason as the attention
                nll.append(F.cross_entropy(x[at: at + n] @ W.t() + bias, tgt[at: at + n], reduction="none"))
                at += n
            nll = torch.cat(nll)
            out[f"{name}_nll"], out[f"{name}_counts"], out[f"{name}_real"] = nll, counts, real
            out[f"loss_{name}"] = nll.mean()
        out["loss"] = self.cfg.text_weight * out["loss_text"] + (1.0 - self.cfg.text_weight) * out["loss_mel"]
        return out

    def evaluate(self, b):
        """The losses of a batch without dropout and without gradient: loss_text, loss_mel, loss (floats: the means over every
        position, as UnifiedVoice.score reports them) and per utterance nll_text / nll_mel over its real positions (its tokens and
        the first stop), as IndexTTS.score_codes reports them."""
        with torch.no_grad():
            o = self._forward(b, False)
        rec = {k: float(o[k].item()) for k in ("loss_text", "loss_mel", "loss")}
        for name in ("text", "mel"):
            nll, at, per = o[f"{name}_nll"].double().cpu(), 0, []
            for n, real in zip(o[f"{name}_counts"], o[f"{name}_real"]):
                per.append(float(nll[at: at + real].mean()))
                at += n
            rec[f"nll_{name}"] = per
        return rec

    def backward(self, b, weight: float = 1.0, accumulate: bool = False, step: int | None = None, micro: int = 0, head_weights=None):
        """One forward and backward of `weight` x loss: the factor gradients land in (accumulate: are added to) the engine's
        gradient buffers.  -> the batch's losses (device scalars).  The dropout masks are drawn from (seed, step, micro).
        head_weights = (w_text, w_mel) in the place of `weight`: the loss is text_weight w_text loss_text + (1 - text_weight) w_mel
        loss_mel -- with w = this batch's share of a larger batch's positions of that head, the micro-batches' gradients add up to
        the larger batch's (a loss is a mean over positions, and the two heads count different positions)."""
        step = self.step_count if step is None else int(step)
        gen = None
        if self.cfg.dropout > 0:
            gen = torch.Generator(device=self.device)
            gen.manual_seed((int(self.cfg.seed) * 1000003 + step) * 1009 + int(micro))
        self._accumulate = bool(accumulate)
        with torch.enable_grad():                    # (whatever the caller's grad mode: inference code turns it off process-wide)
            o = self._forward(b, True, gen)
            if head_weights is None:
                loss = o["loss"] * float(weight)
            else:
                tw = float(self.cfg.text_weight)
                loss = tw * float(head_weights[0]) * o["loss_text"] + (1.0 - tw) * float(head_weights[1]) * o["loss_mel"]
            loss.backward()
        return {k: o[k].detach() for k in ("loss_text", "loss_mel", "loss")}

    def lr_now(self):
        cfg = self.cfg
        return float(cfg.lr) * cosine_with_warmup(self.step_count, int(int(cfg.total_steps) * float(cfg.warmup_ratio)), int(cfg.total_steps))

    def step(self, batch):
        """One optimizer step over a batch, or over a list of batches (gradient accumulation: each weighs 1 / len).  -> report:
        loss_text, loss_mel, loss (the means over the micro-batches), grad_norm (before clipping), lr (group A's), step."""
        from .. import _native_fit as nf
        cfg = self.cfg
        micro = batch if isinstance(batch, (list, tuple)) else [batch]
        if not micro:
            raise ValueError("FitEngine.step: no batch")
        losses = [self.backward(b, 1.0 / len(micro), accumulate=k > 0, micro=k) for k, b in enumerate(micro)]
        norm = math.sqrt(float(nf.sqnorm(self.table).item()))                            # the one float the host reads
        clip = 1.0 if cfg.max_grad_norm is None else min(1.0, float(cfg.max_grad_norm) / (norm + 1e-6))
        lr = self.lr_now()
        nf.adamw_step(self.table, (lr, lr * float(cfg.loraplus_lr_ratio)), (cfg.weight_decay, cfg.weight_decay), self.step_count + 1,
                      clip=clip, beta1=cfg.beta1, beta2=cfg.beta2, eps=cfg.eps)
        self._refresh()
        self.step_count += 1
        rep = {k: float(sum(x[k] for x in losses).item()) / len(micro) for k in ("loss_text", "loss_mel", "loss")}
        rep.update(grad_norm=norm, lr=lr, step=self.step_count)
        return rep


def merged_state_dict(state_dict, adapters, scaling, layers: int):
    """The reference's gpt_finetuned.pth from a voice: a copy of `state_dict` with W + s (B A)^T in the place of every adapted
    Conv1D weight, computed in float64 and stored in the checkpoint's own dtype; every other tensor as it is."""
    out = {k: v.detach().clone() for k, v in state_dict.items()}
    known = {f"gpt.h.{i}.{name}" for i in range(layers) for name in TARGETS}
    bad = sorted(set(adapters) - known)
    if bad:
        raise ValueError(f"save_merged: unknown adapter targets {bad}")
    for key, (A, B) in adapters.items():
        W = out[key + ".weight"]
        A64, B64 = A.detach().to("cpu", torch.float64), B.detach().to("cpu", torch.float64)
        if A64.shape[1] != W.shape[0] or B64.shape[0] != W.shape[1] or A64.shape[0] != B64.shape[1]:
            raise ValueError(f"save_merged: {key}: A {tuple(A.shape)}, B {tuple(B.shape)} do not fit W {tuple(W.shape)}")
        out[key + ".weight"] = (W.to("cpu", torch.float64) + float(scaling) * (B64 @ A64).t()).to(W.dtype)
    return out
