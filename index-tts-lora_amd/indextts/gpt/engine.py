"""GPT-2 acoustic-token decoder engine on the HIP kernels (prefill, cached decode loop, teacher-forced latent pass).

Replaces, for the inference path, HF `GPT2Model` + `GenerationMixin.generate` as wired by the reference in
indextts/gpt/model.py:125-205 (GPT2InferenceModel.forward), :263-286 (build_hf_gpt_transformer) and :459-474
(get_logits).  Host code only does tensor plumbing (torch device memory, streams, CUDA-graph capture/replay); every
FLOP of the transformer runs in libindextts_hip.so.

Data layout in HBM
  * weights: packed MFMA B-fragment blocks (include/indextts_hip.h), dtype T (fp32 parity mode / bf16 speed mode);
    LayerNorm parameters, biases and embedding tables stay fp32.
  * residual stream h: fp32 [rows][D].  T-typed scratch: xn, qkv, attn, ffn.
  * KV cache: T [L][Bmax][H][Smax][64], K and V separate; all rows of a (left-padded) batch share one write position.
  * decode-loop state (int32[8], device): step k, cache position, finished count, arrival counter.
"""
from __future__ import annotations

import itertools
import os
from types import SimpleNamespace

import torch

from .. import _native as nat
from . import voice_pool
from ..utils import quant


KV_TAB = 64   # ITTS_KV_TAB: ring entries of a row's block table


class PagedKV:
    """Paged KV cache of one engine (include/indextts_hip.h, "Paged KV cache"): a block pool per layer, K and V, T
    [L][blocks][H][bs][64]; a block table int32 [rows][64] on the device with a host mirror; a free list.  Block 0 is the
    scratch block: every table entry that maps no live position points at it (a row that has stopped keeps appending its
    stop-token keys there; masked / clamped reads stay inside the pool).  Positions are the decode loop's global positions
    (left-padded rows, one shared write position); the table is a ring over position / bs, so the position counter may grow
    without bound while every row's live window stays under (64 - 2) * bs positions."""

    def __init__(self, L, H, rows, blocks, bs, dtype, device):
        assert bs in (16, 32, 64)
        self.bs, self.shift, self.rows, self.blocks = bs, bs.bit_length() - 1, rows, blocks
        self.kc = torch.zeros(L, blocks, H, bs, 64, dtype=dtype, device=device)
        self.vc = torch.zeros(L, blocks, H, bs, 64, dtype=dtype, device=device)
        self.tab = torch.zeros(rows, KV_TAB, dtype=torch.int32, device=device)
        self.reset()

    def reset(self):
        import numpy as np
        self.tab_h = np.zeros((self.rows, KV_TAB), dtype=np.int32)
        self.free = list(range(self.blocks - 1, 0, -1))     # block 0 = scratch
        self.span = [None] * self.rows                       # per row: [first, last + 1) block INDEX (position >> shift) mapped
        self.dirty = True

    @property
    def window(self):
        """Most positions a row may keep live."""
        return (KV_TAB - 2) * self.bs

    def cover(self, row, lo, hi):
        """Map blocks for positions [lo, hi) of `row` (extends the row's span at its upper end; a new row starts a span)."""
        b0, b1 = lo >> self.shift, ((hi - 1) >> self.shift) + 1
        sp = self.span[row]
        if sp is None:
            sp = self.span[row] = [b0, b0]
        if b1 - sp[0] > KV_TAB - 1:
            raise ValueError(f"paged KV: row {row} would keep {(b1 - sp[0]) * self.bs} positions live (limit {self.window})")
        need = b1 - sp[1]
        if need > 0:
            if need > len(self.free):
                raise RuntimeError("paged KV: the block pool is exhausted")
            import numpy as np
            ids = self.free[-need:][::-1]                   # the blocks pop() would hand out, in that order
            del self.free[-need:]
            self.tab_h[row, (np.arange(sp[1], b1) & (KV_TAB - 1))] = ids
            sp[1] = b1
            self.dirty = True

    def blocks_of(self, lo, hi):
        """Blocks that map positions [lo, hi) of a new row."""
        return ((hi - 1) >> self.shift) - (lo >> self.shift) + 1

    def release(self, row):
        """The row has left: its blocks go back to the pool, its entries to the scratch block."""
        sp = self.span[row]
        if sp is None:
            return
        for bi in range(sp[0], sp[1]):
            self.free.append(int(self.tab_h[row, bi & (KV_TAB - 1)]))
        self.tab_h[row, :] = 0
        self.span[row] = None
        self.dirty = True

    def flush(self):
        """Host mirror -> device table, on the current stream (ordered between the loop's graph replays)."""
        if self.dirty:
            self.tab.copy_(torch.from_numpy(self.tab_h))
            self.dirty = False

    def phys(self, rows, pos):
        """(block, offset) numpy arrays of positions `pos` of table rows `rows` (numpy int arrays of equal length)."""
        import numpy as np
        rows, pos = np.asarray(rows, dtype=np.int64), np.asarray(pos, dtype=np.int64)
        return self.tab_h[rows, (pos >> self.shift) & (KV_TAB - 1)].astype(np.int64), pos & (self.bs - 1)

    def used_blocks(self):
        return self.blocks - 1 - len(self.free)


PER_ROW = {"per_row": True}   # what a loop's `sp` becomes once its rows' settings live in the device table (RowSampling): the
#                               captured step's key carries this marker, never the values


class RowSampling:
    """Per-row sampling settings of one engine: the device table itts_sample_rows reads (uint8 [rows][32], one itts_sample_row
    per decode slot), a host mirror and a dirty flag -- flushed with one copy between graph replays, like PagedKV's block
    table.  The records are data: one captured step serves every assignment of settings to rows."""

    def __init__(self, rows, device):
        import numpy as np
        self.rows = rows
        self.tab = torch.zeros(rows, nat.SAMPLE_ROW_BYTES, dtype=torch.uint8, device=device)
        self.tab_h = np.zeros((rows, nat.SAMPLE_ROW_BYTES), dtype=np.uint8)
        self.dirty = True

    def set(self, rows, settings):
        """Slot rows[j] <- settings[j] (dicts that passed nat.check_sample_row)."""
        if len(rows):
            self.tab_h[list(rows)] = nat.pack_sample_rows(settings)
            self.dirty = True

    def flush(self):
        """Host mirror -> device table, on the current stream (ordered between the loop's graph replays)."""
        if self.dirty:
            self.tab.copy_(torch.from_numpy(self.tab_h))
            self.dirty = False


def admit(kv: PagedKV, rows, items, end, max_new, check_every) -> int:
    """Admission of fed utterances into free decode slots (GPTEngine.decode_refill), host only.  Item j = (prefix [P_j, D],
    stop step) takes slot rows[j] with its prompt + start token at positions [end - P_j - 1, end), and its row is dealt at once
    the blocks of its whole window [pad, end + max_new + check_every): its last token and the steps up to the poll that finds
    it stopped.  Items are admitted in order while that window fits the block table and the free blocks; the first that does
    not -- and every later one -- is not placed.  Returns the number of admitted items."""
    hi = end + max_new + check_every
    for j, (p, _) in enumerate(items):
        pad = end - int(p.shape[0]) - 1
        if hi - pad > kv.window or kv.blocks_of(pad, hi) > len(kv.free):
            return j
        kv.cover(rows[j], pad, hi)
    return len(items)


class LatentCache:
    """The K / V cache of the incremental latent pass (GPTEngine.latent_cache / latent_append): kc / vc of shape
    T [L][rows][H][cap][64], contiguous per layer, and on the host have[row] = the positions row holds and voice[row] = the
    voice they were computed under.  Positions >= have[row] are never read, so reset() clears nothing on the device."""

    @staticmethod
    def nbytes(L, D, rows, cap, dtype):
        return L * 2 * D * cap * rows * torch.empty(0, dtype=dtype).element_size()

    def __init__(self, L, H, rows, cap, dtype, device):
        import numpy as np
        self.rows, self.cap = rows, cap
        self.kc = torch.zeros(L, rows, H, cap, 64, dtype=dtype, device=device)
        self.vc = torch.zeros(L, rows, H, cap, 64, dtype=dtype, device=device)
        self.have = np.zeros(rows, dtype=np.int64)
        self.voice = [None] * rows

    def reset(self, row: int):
        """Row `row` starts a new sequence."""
        self.have[int(row)] = 0
        self.voice[int(row)] = None


class GPTEngine:
    def __init__(self, W: dict, layers: int, model_dim: int, heads: int, dtype=torch.bfloat16, device="cuda",
                 start_mel_token=8192, stop_mel_token=8193, weight_dtype=None, kv_dtype=None):
        assert model_dim == heads * 64, "kernels are specialised for head_dim 64"
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8' (got {kv_dtype!r})")
        # "fp8": the paged KV cache holds one E4M3 byte per element with one power-of-two fp32 scale per (layer, K | V, head)
        # (self.kv_scale); the decode step's attention appends and reads it (itts_attn_decode_kv8), the prefill writes it through
        # itts_kv8_store.  Composes with weight_dtype.  DESIGN.md section 4.11.
        self.kv_dtype = kv_dtype
        if weight_dtype not in (None, "fp8"):
            raise ValueError(f"weight_dtype must be None or 'fp8' (got {weight_dtype!r})")
        # "fp8": the decode step streams E4M3 weights with one fp32 scale per output column (itts_gemm_skinny_w8; utils/quant.py);
        # activations, accumulation, KV cache and statistics stay `dtype`.  DESIGN.md section 4.10.
        self.weight_dtype = weight_dtype
        self.L, self.D, self.H = layers, model_dim, heads
        self.dtype, self.device = dtype, torch.device(device)
        self.start_mel, self.stop_mel = start_mel_token, stop_mel_token
        dev = self.device

        def f32(k):
            return W[k].detach().to(dev, torch.float32).contiguous()

        def packed(w_kn):
            return nat.pack_weight(w_kn.detach().to(dev, dtype).contiguous())

        # Decode-step structure:
        #   "fold" (default for bf16 / f16): LayerNorm folded into the consuming GEMM -- 5 launches per block.  The QKV and FC
        #            GEMMs multiply the RAW residual rows (a T-typed packed copy `hb` of h) by gamma . W and apply the row
        #            statistics, which they compute themselves on the matrix pipe, in their epilogue (csrc/gemm_skinny.hip);
        #            the out-projection and FC2 run without split-K and add into h in their epilogue (one owner per element,
        #            deterministic), storing hb beside it.  One [LayerNorm + LayerNorm] launch per token is left (ln_f, final_norm).
        #   "launch": every [residual-reduce + LayerNorm] is a launch of its own behind a split-K GEMM -- 7 launches per block.
        #            fp32 parity mode and engines with runtime LoRA adapters (whose (x A) B term rides on the reduce launch).
        # Forms measured and removed in rounds 1-3: LayerNorm in the consumer GEMM's PROLOGUE, LN rows produced by extra
        # workgroups of the consumer's launch, a reducer tail inside the split-K launches.
        self.decode_mode = os.environ.get("ITTS_DECODE_MODE", "fold" if dtype != torch.float32 else "launch")
        if self.decode_mode not in ("fold", "launch"):
            raise ValueError("ITTS_DECODE_MODE must be 'fold' or 'launch'")
        if dtype == torch.float32:
            self.decode_mode = "launch"
        if weight_dtype == "fp8":
            if dtype == torch.float32:
                raise ValueError("weight_dtype='fp8' needs 16-bit activations (dtype bf16 or f16): the FP8 GEMM converts to them")
            if self.decode_mode != "fold":
                raise ValueError("weight_dtype='fp8' needs the 'fold' decode step (ITTS_DECODE_MODE=launch runs split-K GEMMs, "
                                 "which the FP8 forms do not have)")
        if kv_dtype == "fp8":
            if dtype == torch.float32:
                raise ValueError("kv_dtype='fp8' needs 16-bit activations (dtype bf16 or f16): the FP8 KV kernels are built for them")
            if self.decode_mode != "fold":
                raise ValueError("kv_dtype='fp8' needs the 'fold' decode step (ITTS_DECODE_MODE=launch is not built for the FP8 KV cache)")
        # launch geometry of the two GEMMs that run without split-K in "fold" mode (rows per workgroup, 16-wave workgroups)
        self.fold_rows = [int(v) for v in os.environ.get("ITTS_FOLD_ROWS", "16,16").split(",")]   # out-projection, FC2
        self.fold_rows_consumers = int(os.environ.get("ITTS_FOLD_ROWS_C", "32"))   # QKV' / FC' rows per workgroup when a step has > 32 rows
        self.fold_wide = os.environ.get("ITTS_FOLD_WIDE", "0") == "1"   # measured equal (836.7 / 840.6 us per token)
        # T-typed activations of the decode step (xn, attention output, MLP hidden) live in the packed fragment layout
        # (include/indextts_hip.h): the GEMMs read them as contiguous 1-KiB blocks.  ITTS_PACKED_ACT=0: row-major (same bits).
        self.pa = os.environ.get("ITTS_PACKED_ACT", "1") == "1"
        # beam search: KV rows follow their beams through a row TABLE read by the attention kernel ("table", no cache bytes
        # move) or by permuting the cache rows in place ("copy": itts_beam_reorder_kv, the reference form of
        # GPT2InferenceModel._reorder_cache, model.py:207-218; 1 ms per token at 32 x 3 rows)
        # num_beams = 1: the KV cache is PAGED (block pool + per-row block table, class PagedKV): rows hold only the blocks their
        # own window needs, and continuous batching (decode_refill) hands the blocks of a row that has stopped to the utterance
        # that takes its slot -- the loop runs for as long as the queue lasts inside a fixed pool.  ITTS_PAGED_KV=0: contiguous
        # [rows][H][smax][64] strips (what beam search uses: its per-position row table addresses whole rows).
        self.paged = os.environ.get("ITTS_PAGED_KV", "1") == "1"
        if kv_dtype == "fp8" and not self.paged:
            raise NotImplementedError("the FP8 KV cache (kv_dtype='fp8') is built for the paged cache only (ITTS_PAGED_KV=0 asks for "
                                      "the contiguous one)")
        # one scale per (layer, K | V, head), device data the kernels read: never part of a graph key.  1.0 until set_kv_scales /
        # calibrate_kv_scales.
        self.kv_scale = torch.ones(layers, 2, heads, dtype=torch.float32, device=self.device) if kv_dtype == "fp8" else None
        self.kv = None            # PagedKV of the batch in flight (None: contiguous cache)
        self.beam_kv = os.environ.get("ITTS_BEAM_KV", "table")
        self._kv_rows = None   # the table of the beam decode in progress (None outside decode_beam)
        self._shared_prefix = None   # (B, num_beams) after prefill(beams=n): the prompt's K/V exists once per batch element
        self.max_rows_per_launch = 16 if dtype == torch.float32 else 96   # rows one skinny-GEMM launch covers

        # Rows that have emitted their stop token are left out of the decode attention (the sampler pads them with the stop
        # token whatever their logits are).  Their logits -- decode(return_logits=True) -- are then UNDEFINED from the step
        # after their stop on; every other row is untouched (all later stages are per row).  False: compute them anyway.
        self.skip_finished = True
        self._W = W          # kept (by reference) for attach_lora: the engine itself only holds packed copies
        self.lora = False
        self.bank = None     # per-row adapter bank (attach_lora_bank): n, rp, Kx and the signature the graph key carries
        self._ids_host = None   # adapter id per row of the batch the last prefill() cached
        self._mix_host = None   # ... or, prefilled with adapter_mix, every row's mix (check_adapter_mix); at most one of the two is set
        self.layers = []

        def folded(ln, wkey, bkey):
            """LN(h; gamma, beta) W + b = rstd (h W' - mean c) + d:  W' = T(gamma . W) packed, c = column sums of the ROUNDED W'
            (so that a constant row cancels exactly), d = beta W + b.  Sums in float64, stored fp32."""
            Wm = W[wkey].detach().to(dev, torch.float64)
            g, bt = ln[0].to(torch.float64), ln[1].to(torch.float64)
            Wr = (g[:, None] * Wm).to(torch.float32).to(dtype)
            c = Wr.to(torch.float64).sum(0).to(torch.float32).contiguous()
            d = (bt @ Wm + W[bkey].detach().to(dev, torch.float64)).to(torch.float32).contiguous()
            return nat.pack_weight(Wr.contiguous()), c, d

        def w8(w_kn):
            """fp64 [K, N] -> (packed E4M3 image, fp32 scales [N], the dequantised matrix fp64): what the decode step streams, and
            the values every other pass of this engine must see."""
            codes, scale = quant.quantize_e4m3_cols(w_kn)
            return nat.pack_weight_w8(codes), scale.contiguous(), quant.dequantize(codes, scale)

        def folded_w8(l, tag, ln, wkey, bkey):
            """The folded form over FP8 weights: gamma . W is what is quantised; c = scale . (column sums of the decoded codes), in
            float64, so a constant row still cancels; d = beta W + b from the unquantised W (an fp32 vector, like every bias).
            The big-M passes get the SAME weight values: LayerNorm without affine (ones, zeros), then x @ T(dequantised gamma . W)
            + d -- the identity above with rstd (h - mean) formed by the LayerNorm launch."""
            Wm = W[wkey].detach().to(dev, torch.float64)
            g, bt = l[ln][0].to(torch.float64), l[ln][1].to(torch.float64)
            l["wf_" + tag], l["s_" + tag], deq = w8(g[:, None] * Wm)
            l["c_" + tag] = deq.sum(0).to(torch.float32).contiguous()
            l["d_" + tag] = (bt @ Wm + W[bkey].detach().to(dev, torch.float64)).to(torch.float32).contiguous()
            l[ln] = (torch.ones_like(l[ln][0]), torch.zeros_like(l[ln][1]))
            l["w_" + tag], l["b_" + tag] = packed(deq), l["d_" + tag]
        for i in range(layers):
            p = f"gpt.h.{i}."
            d = dict(
                ln1=(f32(p + "ln_1.weight"), f32(p + "ln_1.bias")),
                ln2=(f32(p + "ln_2.weight"), f32(p + "ln_2.bias")),
                b_qkv=f32(p + "attn.c_attn.bias"), b_o=f32(p + "attn.c_proj.bias"),
                b_fc=f32(p + "mlp.c_fc.bias"), b_pr=f32(p + "mlp.c_proj.bias"),
            )
            if weight_dtype != "fp8":   # (an FP8 engine packs 16-bit copies of the DEQUANTISED weights below: each weight once)
                d.update(w_qkv=packed(W[p + "attn.c_attn.weight"]), w_o=packed(W[p + "attn.c_proj.weight"]),
                         w_fc=packed(W[p + "mlp.c_fc.weight"]), w_pr=packed(W[p + "mlp.c_proj.weight"]))
            if weight_dtype == "fp8":
                folded_w8(d, "qkv", "ln1", p + "attn.c_attn.weight", p + "attn.c_attn.bias")
                folded_w8(d, "fc", "ln2", p + "mlp.c_fc.weight", p + "mlp.c_fc.bias")
                for tag, wkey in (("o", p + "attn.c_proj.weight"), ("pr", p + "mlp.c_proj.weight")):
                    d["w8_" + tag], d["s_" + tag], deq = w8(W[wkey].detach().to(dev, torch.float64))
                    d["w_" + tag] = packed(deq)       # the prefill / latent passes: 16-bit copies of the dequantised values
            elif self.decode_mode == "fold":
                d["wf_qkv"], d["c_qkv"], d["d_qkv"] = folded(d["ln1"], p + "attn.c_attn.weight", p + "attn.c_attn.bias")
                d["wf_fc"], d["c_fc"], d["d_fc"] = folded(d["ln2"], p + "mlp.c_fc.weight", p + "mlp.c_fc.bias")
            self.layers.append(d)
        self.ln_f = (f32("gpt.ln_f.weight"), f32("gpt.ln_f.bias"))
        self.final_norm = (f32("final_norm.weight"), f32("final_norm.bias"))
        self.V = W["mel_head.weight"].shape[0]
        if weight_dtype == "fp8":   # every use of the head is a skinny GEMM: no 16-bit copy
            self.w_head, self.s_head, _ = w8(W["mel_head.weight"].detach().to(dev, torch.float64).t())
        else:
            self.w_head, self.s_head = packed(W["mel_head.weight"].t()), None
        self.b_head = f32("mel_head.bias")
        self.mel_emb = f32("mel_embedding.weight")
        self.mel_pos = f32("mel_pos_embedding.emb.weight")
        self.text_emb = f32("text_embedding.weight")
        self.text_pos = f32("text_pos_embedding.emb.weight")
        self.extra_ids = torch.tensor([1, start_mel_token], dtype=torch.int32, device=dev)  # fake prefix ids (model.py:658-667)
        self._cap_b = self._cap_s = 0
        self._kv_pool = None      # the PagedKV object kept across batches (re-made when it has to grow)
        self._graphs = {}
        # split-K of the two N=1280 GEMMs of a block (80 column tiles): 3 -> 80 x 3 = 240 workgroups of one tile; 6 -> 40 x 6 = 240
        # workgroups of TWO tiles, whose waves fetch each activation fragment once for both (a third less load traffic per CU)
        self.KSPLIT = int(os.environ.get("ITTS_KSPLIT", "3"))
        self.force_eager = False  # measurement aid: launch every kernel eagerly
        self.share_prefix = os.environ.get("ITTS_SHARE_PREFIX", "1") != "0"   # prefill(shared_rows=C): compute the shared rows once
        self.share_kv_reads = os.environ.get("ITTS_SHARE_KV_READS", "1") != "0"   # ... and let the decode attention read them from row 0
        self._sink = torch.zeros(4, dtype=torch.int32, device=dev)
        # the packed weights one decode step streams (FP8: one byte per weight; the scales, like the biases, are not counted)
        step_w = ("wf_qkv", "w8_o", "wf_fc", "w8_pr") if weight_dtype == "fp8" else ("w_qkv", "w_o", "w_fc", "w_pr")
        self.weight_bytes = sum(l[k].numel() * l[k].element_size() for l in self.layers for k in step_w) + self.w_head.numel()

    # ------------------------------------------------------------------------------------------------ runtime LoRA
    def attach_lora(self, adapters: dict, scaling: float):
        """Unmerged LoRA adapters at run time (the reference always merges them before saving, train.py:802-832; this is the
        north_star's "LoRA A.B fused into the output projection").  `adapters`: {"gpt.h.{i}.attn.c_proj": (A, B), ...} with
        the peft tensors of a Conv1D target (fan_in_fan_out=True): A = lora_A.weight [r, in], B = lora_B.weight [out, r];
        y = x W + (x A^T) B^T * scaling, scaling = lora_alpha / r (train.py:555-563).
          * output projections (attn.c_proj, mlp.c_proj): stay UNMERGED in the decode loop -- A^T * scaling rides along as
            16*ceil(r/16) extra output columns of the packed weight (the split-K GEMM produces x A next to x W), and the
            [residual-reduce + LayerNorm] launch that follows adds (x A) B^T: no extra launch, no merged weight copy;
          * attn.c_attn / mlp.c_fc adapters, and every adapter in the large-M passes (prefill, latent), are merged into
            packed copies here (their GEMMs have no reduce stage to carry the correction)."""
        dev, T, D = self.device, self.dtype, self.D
        W = self._W
        if adapters and self.kv_dtype is not None:
            raise NotImplementedError("attach_lora(): LoRA with the FP8 KV cache (kv_dtype='fp8') is not built: adapters run the "
                                      "7-launch decode step, whose QKV epilogue appends 16-bit keys")
        if adapters and self.weight_dtype is not None:
            raise ValueError("attach_lora(): LoRA on an FP8 base is not built (weight_dtype='fp8'): the adapters' extra columns and "
                             "merged copies are 16-bit operands")

        def f32(k):
            return W[k].detach().to(dev, torch.float32)

        def packed(w):
            return nat.pack_weight(w.to(T).contiguous())

        if adapters and self.bank is not None:
            raise ValueError("attach_lora(): an adapter bank is attached (detach_lora_bank() first): one or the other")
        self.detach_lora()   # every attach starts from the base weights: nothing of an earlier adapter set survives
        if not adapters:     # attach_lora(None) = detach
            return
        for i, l in enumerate(self.layers):
            p = f"gpt.h.{i}."
            for name, wkey in (("attn.c_attn", "w_qkv"), ("mlp.c_fc", "w_fc")):
                if p + name in adapters:
                    A, Bm = (t.detach().to(dev, torch.float32) for t in adapters[p + name])
                    l[wkey + "_base"] = l[wkey]
                    l[wkey] = packed(f32(p + name + ".weight") + (A.t() @ Bm.t()) * scaling)
            for name, wkey, tag in (("attn.c_proj", "w_o", "o"), ("mlp.c_proj", "w_pr", "pr")):
                if p + name not in adapters:
                    continue
                A, Bm = (t.detach().to(dev, torch.float32) for t in adapters[p + name])
                r = A.shape[0]
                if r > 64:
                    raise ValueError("runtime LoRA supports rank <= 64")
                rp = (r + 15) // 16 * 16
                base = f32(p + name + ".weight")                                  # [K, D]
                ext = torch.zeros(base.shape[0], D + rp, dtype=torch.float32, device=dev)
                ext[:, :D] = base
                ext[:, D:D + r] = A.t() * scaling
                l[wkey + "_lora"] = packed(ext)                                   # decode: [W | A^T s], N = D + rp
                l["lora_b_" + tag] = Bm.t().contiguous()                          # [r, D] fp32, applied by ln_reduce
                l["lora_n_" + tag] = D + rp
                l[wkey + "_merged"] = packed(base + (A.t() @ Bm.t()) * scaling)   # large-M passes
        self.lora = True
        self._graphs.clear()
        if hasattr(self, "slab") and self.slab.shape[2] < D + 64:
            self._cap_b = self._cap_s = 0   # the slabs need room for the extra columns: reallocate on the next prefill

    def detach_lora(self):
        """Back to the base weights: drops every adapter-derived entry (extra-column projections, merged copies, B factors)
        and the graphs captured over them.  Only this engine changes: a fork holds its own layer dicts."""
        for l in self.layers:
            for k in [k for k in l if k.endswith("_lora") or k.endswith("_merged") or k.startswith("lora_")]:
                del l[k]
            for wkey in ("w_qkv", "w_fc"):
                if wkey + "_base" in l:
                    l[wkey] = l.pop(wkey + "_base")
        self.lora = False
        self._graphs.clear()

    def extract_lora(self, tuned_state_dict: dict, max_rank: int = 16, gap: float = 8.0, seed: int = 0, ignore_other: bool = False):
        """The LoRA a MERGED fine-tuned checkpoint of this engine's base holds (what train.py saves: merge_and_unload(), fp16), as
        (adapters, 1.0, report): adapters in the attach_lora format -- what attach_lora_bank, VoicePool.add and add_voice take --
        and per target the rank found, sigma_r, sigma_{r+1} and their ratio.  The base is this engine's own checkpoint; the
        difference is reached only through ittv_delta_project launches (gpt/voice_extract.py).  ValueError
        before any launch: a shape mismatch, tensors outside the 4 x layers targets that differ (ignore_other=True overrides); and
        per target: no singular-value ratio of at least `gap`, or a rank above max_rank -- a full fine-tune, or the wrong base.  A
        target that did not change names no adapter.  Nothing of the engine changes."""
        from indextts.gpt import voice_extract
        return voice_extract.extract(self._W, tuned_state_dict, self.L, voice_extract.DeviceDelta(self.device), max_rank=max_rank,
                                     gap=gap, seed=seed, ignore_other=ignore_other)

    # ------------------------------------------------------------------------------------------------ adapter bank
    BANK_TARGETS = (("attn.c_attn", "w_qkv"), ("attn.c_proj", "w_o"), ("mlp.c_fc", "w_fc"), ("mlp.c_proj", "w_pr"))

    def attach_lora_bank(self, bank):
        """A bank of LoRA adapter sets, one per voice, chosen PER ROW of a batch (self.adapter_ids / prefill(adapter_ids=...); -1 =
        the base voice).  `bank`: a list of (adapters, scaling) in the attach_lora format; every set may name any of the four
        targets of any layer, ranks may differ (each is zero-padded to rp = 16 * ceil(r_max / 16)).
        For a row with adapter a:  y = x W + s_a (x A_a^T) B_a^T = [x | u] [W ; B_bank^T], u = the row's Kx-wide shrink vector
        (itts_lora_shrink: s_a x A_a^T in the slot of adapter a, zeros elsewhere), B_bank^T = every adapter's B^T stacked.  The
        GEMMs run unchanged over K + Kx, so the LoRA term is in their accumulator before the bias, the GELU and the K/V append.
        Per layer and target this keeps A_bank T [n, rp, K] and a packed copy of [W ; B_bank^T] (the packed layout has the
        k-step innermost: extending K is a re-pack, i.e. a second copy of the block weights).  A target no adapter names keeps
        its base weight and gets no shrink launch.  The decode step runs in "launch" form (the folded GEMMs take their
        LayerNorm statistics over K on the matrix pipe; the shrink needs xn = LN(h) as an operand anyway)."""
        self._bank_refusals("attach_lora_bank")
        bank = [(dict(ad), float(sc)) for ad, sc in bank]
        n = len(bank)
        if n < 1:
            raise ValueError("attach_lora_bank(): the bank is empty")
        known = {f"gpt.h.{i}.{name}" for i in range(self.L) for name, _ in self.BANK_TARGETS}
        for ad, _ in bank:
            bad = sorted(set(ad) - known)
            if bad:
                raise ValueError(f"attach_lora_bank(): unknown adapter targets {bad}")
        ranks = [int(A.shape[0]) for ad, _ in bank for A, _ in ad.values()]
        if not ranks:
            raise ValueError("attach_lora_bank(): no adapter names a target")
        if max(ranks) > 64:
            raise ValueError("the adapter bank supports rank <= 64")
        rp = (max(ranks) + 15) // 16 * 16
        names = {wkey: name for name, wkey in self.BANK_TARGETS}
        targets = [(i, wkey) for i in range(self.L) for _, wkey in self.BANK_TARGETS
                   if any(f"gpt.h.{i}.{names[wkey]}" in ad for ad, _ in bank)]
        self._bank_build("attach_lora_bank", n, rp, targets, bank)

    def _bank_refusals(self, who):
        """What an adapter bank -- fixed (attach_lora_bank) or paged (attach_lora_pool) -- cannot be attached to."""
        if self.kv_dtype is not None:
            raise NotImplementedError(f"{who}(): LoRA with the FP8 KV cache (kv_dtype='fp8') is not built: the bank runs "
                                      "the 7-launch decode step, whose QKV epilogue appends 16-bit keys")
        if self.weight_dtype is not None:
            raise ValueError(f"{who}(): LoRA on an FP8 base is not built (weight_dtype='fp8'): the bank's K-extended "
                             "weight mixes base rows and adapter rows in one packed operand")
        if self.lora:
            raise ValueError(f"{who}(): single adapters are attached (attach_lora(None) first): one or the other")
        if not self.pa:
            raise ValueError(f"{who}(): the bank needs the packed activation layout (ITTS_PACKED_ACT=1)")

    def _bank_build(self, who, n, rp, targets, bank=()):
        """The bank's structure for n slots of padded rank rp on `targets` [(layer, weight key)]: per target A_bank T [n, rp, K] and
        the packed [W ; B_bank^T], filled from `bank` [(adapters, scaling)] -- slot a <- bank[a]; slots beyond it stay zero."""
        Kx = nat.lora_kx(n, rp)
        if Kx > 512:
            raise ValueError(f"{who}(): {n} adapters of padded rank {rp} need {Kx} extra operand columns (limit 512)")
        dev, T, W = self.device, self.dtype, self._W
        names = {wkey: name for name, wkey in self.BANK_TARGETS}
        self.detach_lora_bank()
        for i, wkey in targets:
            l, key = self.layers[i], f"gpt.h.{i}.{names[wkey]}"
            base = W[key + ".weight"].detach().to(dev, torch.float32)              # [K, N]
            K, N = base.shape
            a_bank = torch.zeros(n, rp, K, dtype=torch.float32, device=dev)
            ext = torch.zeros(K + Kx, N, dtype=torch.float32, device=dev)
            ext[:K] = base
            for a, (ad, sc) in enumerate(bank):
                if key in ad:
                    A, Bm = (t.detach().to(dev, torch.float32) for t in ad[key])
                    r = A.shape[0]
                    if A.shape != (r, K) or Bm.shape != (N, r):
                        raise ValueError(f"{who}(): {key} of adapter {a}: A must be [r, {K}] and B [{N}, r]")
                    a_bank[a, :r] = A * sc                                           # the scaling rides on A, folded in at fp32
                    ext[K + a * rp:K + a * rp + r] = Bm.t()
            l["bank_a_" + wkey] = a_bank.to(T).contiguous()
            l["bank_" + wkey] = nat.pack_weight(ext.to(T).contiguous())
        self.bank = SimpleNamespace(n=n, rp=rp, Kx=Kx, sig=(n, rp, tuple((i, k) for i, k in targets)), pool=None)
        self._graphs.clear()
        if hasattr(self, "xn") and self.xn.shape[1] < self.D + Kx:
            self._cap_b = self._cap_s = 0   # xn / a / f need room for the shrink columns: reallocate on the next prefill

    def attach_lora_pool(self, pool, slots: int):
        """The adapter bank as a CACHE over a voice pool (gpt/voice_pool.py): exactly the structure
        attach_lora_bank builds for `slots` voices of padded rank pool.rp on pool.targets, with all-zero extension rows and zero
        bank_a_*; same refusals, exclusive with attach_lora_bank (detach_lora_bank() detaches either).  From here on adapter_ids /
        adapter_mix name POOL VOICE IDS wherever the engine takes voices: they are checked against the pool, the named voices
        are made resident (voice_pool.Residency: residents keep their slot, misses take empty slots, then the least recently
        used unpinned one), every miss is paged in -- per (layer, target) one strided device copy of its B-image into the
        slot's run of bank_w* and one contiguous copy of its A-image into bank_a_*[slot], on the current stream, i.e. between
        graph replays like PagedKV.flush, no host synchronisation -- and the ids are rewritten to slot numbers before the
        device tables are packed.  bank.sig stays (slots, rp, targets): one captured step serves every voice of the pool;
        pool.add / pool.remove need no re-attach and clear no graph.
        Pins (counts): prefill() pins its batch's voices until the next prefill() or the detach; the refill loop pins a row's
        voices from its admission until the loop is resumed behind the poll that reported the row stopped -- so the passes a
        stream runs for that last poll (latent pass, latent-cache append) find them resident -- and a fed item whose voices do
        not fit beside the pinned ones waits (voice_pool.admit_voices), its voices guarded against pool.remove meanwhile.  Any other call acquires its voices at once and launches
        in stream order behind its page-ins, which is all a pin for its own duration would give."""
        self._bank_refusals("attach_lora_pool")
        if self.bank is not None:
            raise ValueError("attach_lora_pool(): an adapter bank or pool is attached (detach_lora_bank() first): one or the other")
        if (pool.L, pool.D, pool.dtype, pool.device) != (self.L, self.D, self.dtype, self.device):
            raise ValueError("attach_lora_pool(): the pool was made for another engine (layers, width, dtype or device differ)")
        slots = int(slots)
        if slots < 1:
            raise ValueError("attach_lora_pool(): at least one slot")
        self._bank_build("attach_lora_pool", slots, pool.rp, list(pool.targets))
        self._pool_adopt(pool, voice_pool.Residency(slots))

    def _pool_adopt(self, pool, res):
        """This engine's bank_* tensors page voices of `pool` under the bookkeeping `res`."""
        self.bank.pool, self.bank.res, self.bank.deferrals = pool, res, 0
        pool._residencies.add(res)

    def _pool(self):
        bank = self.bank
        return None if bank is None else getattr(bank, "pool", None)

    def pool_resident(self):
        """slot -> the pool voice resident there, or None."""
        if self._pool() is None:
            raise ValueError("pool_resident(): no voice pool is attached (attach_lora_pool)")
        return self.bank.res.resident()

    def pool_stats(self):
        """Page-ins (loads), acquires that found their voice resident (hits), evictions, and fed items that had to wait for a slot."""
        if self._pool() is None:
            raise ValueError("pool_stats(): no voice pool is attached (attach_lora_pool)")
        r = self.bank.res
        return {"loads": r.loads, "hits": r.hits, "evictions": r.evictions, "deferrals": self.bank.deferrals}

    def _page_in(self, loads):
        """[(slot, voice)] -> the voices' images into the slots, on the current stream."""
        bank, es = self.bank, torch.empty(0, dtype=self.dtype).element_size()
        for slot, voice in loads:
            for i, wkey in bank.pool.targets:
                l = self.layers[i]
                a_img, b_img = bank.pool.images(voice, (i, wkey))
                K, N = voice_pool.target_shape(wkey, self.D)
                NT, stride, off, run = voice_pool.span(K, N, bank.Kx, slot, bank.rp, es)
                l["bank_" + wkey].view(NT, stride)[:, off:off + run].copy_(b_img)
                l["bank_a_" + wkey][slot].copy_(a_img)

    def _slots(self, ids, mix, pin=None):
        """Checked (ids, mix) in pool voice ids -> the same in bank slot numbers, with every named voice resident and paged in
        (no pool: unchanged).  pin (a list): the voices are pinned and appended to it; the caller unpins them."""
        if self._pool() is None:
            return ids, mix
        res = self.bank.res
        named = [v for v in ids if v >= 0] if mix is None else [i for row in mix for i, _ in row]
        named = list(dict.fromkeys(named))
        self._page_in(res.acquire(named))
        if pin is not None:
            res.pin(named)
            pin.extend(named)
        at = res.slot_of
        if mix is None:
            return [-1 if v < 0 else at[v] for v in ids], None
        return None, [tuple(sorted((at[i], w) for i, w in row)) for row in mix]

    def batch_fit(self, voices) -> int:
        """How many leading rows of `voices` (checked ids, or normalised mixes) one batch can hold: with a voice pool, as many as
        name no more distinct voices than the bank has slots (at least one: a single row always fits); all of them otherwise."""
        pool = None if self.bank is None else getattr(self.bank, "pool", None)
        if pool is None:
            return len(voices)
        seen = set()
        for j, v in enumerate(voices):
            named = {i for i, _ in v} if isinstance(v, tuple) else {int(v)} - {-1}
            if len(seen | named) > self.bank.n:
                return j
            seen |= named
        return len(voices)

    def _unpin_prefill(self):
        held, self._prefill_pins = getattr(self, "_prefill_pins", None), None
        if held and self._pool() is not None:
            self.bank.res.unpin(held)

    def detach_lora_bank(self):
        """Back to the base weights: drops the bank's A factors and extended weights and the graphs captured over them.  Only this
        engine changes: a fork holds its own layer dicts.  Detaches a voice pool too (attach_lora_pool): its pins go with it."""
        if self._pool() is not None:
            self.bank.pool._residencies.discard(self.bank.res)
        self._prefill_pins = None
        for l in self.layers:
            for k in [k for k in l if k.startswith("bank_")]:
                del l[k]
        self.bank = None
        self._ids_host = None
        self._mix_host = None
        if getattr(self, "adapter_ids", None) is not None:
            self.adapter_ids.fill_(-1)
        if getattr(self, "adapter_mix", None) is not None:
            self.adapter_mix.copy_(self._mix_records([()] * self.adapter_mix.shape[0]))
        self._graphs.clear()

    def _row_adapters(self, adapter_ids, B, queue=False):
        """The batch's adapter ids as host ints, checked before anything is launched (None without a bank; all -1 when a bank is
        attached and the caller names none).  With a voice pool the ids are pool voice ids: each must be alive, and -- unless the
        rows are a queue's (queue=True), which need not be resident together -- the distinct ones at most the slots."""
        if adapter_ids is None:
            return None if self.bank is None else [-1] * B
        if self.bank is None:
            raise ValueError("adapter_ids were given but no adapter bank is attached (attach_lora_bank)")
        ids = [int(v) for v in (adapter_ids.tolist() if torch.is_tensor(adapter_ids) else adapter_ids)]
        if len(ids) != B:
            raise ValueError(f"adapter_ids holds {len(ids)} ids for a batch of {B}")
        pool = getattr(self.bank, "pool", None)   # (read off the bank: these checks also run over engines that hold nothing else)
        if pool is not None:
            gone = [v for v in ids if v != -1 and not pool.alive(v)]
            if gone:
                raise ValueError(f"adapter_ids must be -1 or voices of the pool: {gone} are not (never added, or removed)")
            if not queue and len({v for v in ids if v >= 0}) > self.bank.n:
                raise ValueError(f"adapter_ids name {len({v for v in ids if v >= 0})} distinct voices, the pool is attached with "
                                 f"{self.bank.n} slots")
        elif any(v < -1 or v >= self.bank.n for v in ids):
            raise ValueError(f"adapter_ids must lie in [-1, {self.bank.n}): {ids}")
        return ids

    def check_adapter_mix(self, mix, B, queue=False):
        """The batch's adapter mixes, normalised and checked on the host before anything is launched: one tuple of up to four
        (id, weight) per row, sorted by id (the order of a record's entries moves no bit of the result).  Every element of `mix` is
        None or -1 (the base voice), an int id (that adapter at weight 1), a {id: weight} dict or a sequence of (id, weight).
        ValueError: no bank attached, a wrong number of rows, an id outside [0, n), a repeated id within a row, more than four
        entries, a weight that is not finite.  With a voice pool the ids are pool voice ids: each must be alive, a mix holds at
        most as many entries as the pool has slots, and with queue=False (the rows of one batch) all rows together name at most
        that many distinct voices."""
        import math
        import numbers
        if self.bank is None:
            raise ValueError("adapter_mix was given but no adapter bank is attached (attach_lora_bank)")
        mix = mix.tolist() if torch.is_tensor(mix) else list(mix)
        if len(mix) != B:
            raise ValueError(f"adapter_mix holds {len(mix)} mixes for a batch of {B}")
        pool = getattr(self.bank, "pool", None)
        out = []
        for b, el in enumerate(mix):
            if el is None or (isinstance(el, numbers.Integral) and int(el) == -1):
                out.append(())
                continue
            if isinstance(el, numbers.Integral):
                pairs = [(el, 1.0)]
            elif isinstance(el, dict):
                pairs = list(el.items())
            else:
                try:
                    pairs = [(i, w) for i, w in el]
                except (TypeError, ValueError):
                    raise ValueError(f"adapter_mix[{b}]: a mix is None, -1, an id, a {{id: weight}} dict or a sequence of (id, weight) "
                                     f"(got {el!r})") from None
            if len(pairs) > nat.LORA_MIX_ENTRIES:
                raise ValueError(f"adapter_mix[{b}]: a mix holds at most {nat.LORA_MIX_ENTRIES} entries (got {len(pairs)})")
            if pool is not None and len(pairs) > self.bank.n:
                raise ValueError(f"adapter_mix[{b}]: a mix of {len(pairs)} voices cannot be resident in the pool's {self.bank.n} slots")
            row = []
            for i, w in pairs:
                if pool is not None:
                    if not isinstance(i, numbers.Integral) or not pool.alive(int(i)):
                        raise ValueError(f"adapter_mix[{b}]: ids must be voices of the pool (got {i!r}: never added, or removed)")
                elif not isinstance(i, numbers.Integral) or not 0 <= int(i) < self.bank.n:
                    raise ValueError(f"adapter_mix[{b}]: ids must lie in [0, {self.bank.n}) (got {i!r})")
                if not isinstance(w, numbers.Real) or not math.isfinite(w):
                    raise ValueError(f"adapter_mix[{b}]: the weight of adapter {int(i)} must be a finite number (got {w!r})")
                row.append((int(i), float(w)))
            if len({i for i, _ in row}) != len(row):
                raise ValueError(f"adapter_mix[{b}]: adapter ids repeat within the row: {[i for i, _ in row]}")
            out.append(tuple(sorted(row)))
        if pool is not None and not queue:
            distinct = {i for row in out for i, _ in row}
            if len(distinct) > self.bank.n:
                raise ValueError(f"adapter_mix names {len(distinct)} distinct voices, the pool is attached with {self.bank.n} slots")
        return out

    def _voices(self, adapter_ids, adapter_mix, B, queue=False):
        """(ids, mix) of a batch, checked: adapter ids (_row_adapters) or -- exclusive -- adapter mixes (check_adapter_mix).
        queue: the rows are a queue's utterances, not one batch (a voice pool then places no bound on the distinct voices)."""
        if adapter_mix is None:
            return self._row_adapters(adapter_ids, B, queue), None
        if adapter_ids is not None:
            raise ValueError("adapter_ids and adapter_mix are mutually exclusive: a row is an id or a mix (an int in adapter_mix is "
                             "that adapter at weight 1)")
        return None, self.check_adapter_mix(adapter_mix, B, queue)

    def _mix_records(self, mixes):
        """uint8 device tensor [len(mixes), 32]: the itts_lora_mix_row records of normalised mixes."""
        return torch.from_numpy(nat.pack_lora_mix(mixes)).to(self.device)

    def _row_mix(self, mixes, rows_per_element):
        """Element b's record repeated over its rows (the large-M passes): the counterpart of _row_ids."""
        import numpy as np
        return torch.from_numpy(np.repeat(nat.pack_lora_mix(mixes), np.asarray(rows_per_element, dtype=np.int64), axis=0)).to(self.device)

    def _row_voices(self, ids, mix, rows_per_element):
        """Keyword arguments of _big_m_layers / _blocks_full for a batch's checked (ids, mix)."""
        if mix is not None:
            return dict(row_mix=self._row_mix(mix, rows_per_element))
        return dict(row_ids=None if ids is None else self._row_ids(ids, rows_per_element))

    def _row_ids(self, ids, rows_per_element):
        """int32 device tensor: element b's adapter id repeated over its rows (the large-M passes)."""
        import numpy as np
        return torch.from_numpy(np.repeat(np.asarray(ids, dtype=np.int32), np.asarray(rows_per_element, dtype=np.int64))).to(self.device)

    def fork(self) -> "GPTEngine":
        """A second engine over the SAME packed weights (read-only, shared tensors) with its own KV cache, scratch buffers,
        loop state, captured graphs and per-layer dicts: what a concurrent request needs (infer.RequestPool).  A fork keeps
        the adapter state it was forked with; attach_lora / detach_lora on one engine never changes another.
        A fork of an engine with a voice pool (attach_lora_pool) shares the pool's images, which are read-only, but CLONES the
        bank_* tensors -- a page-in on one engine must not rewrite another's weights -- and keeps its own Residency: that costs a
        second copy of the block weights (K-extended) per fork, about 1 GB at 24 layers x 1280, 16-bit."""
        import copy
        e = copy.copy(self)
        e.layers = [dict(l) for l in self.layers]
        if self._pool() is not None:
            # page-ins rewrite bank_*: the fork gets its own copies and its own residency (the arrangement it was forked with, no pins)
            for l in e.layers:
                for k in [k for k in l if k.startswith("bank_")]:
                    l[k] = l[k].clone()
            e.bank = copy.copy(self.bank)
            e._pool_adopt(self.bank.pool, self.bank.res.copy_unpinned())
            e._prefill_pins = None
        e._cap_b = e._cap_s = 0
        e.kv = None
        e._kv_pool = None
        e._graphs = {}
        e._beam_cap = (0, 0, 0)
        e._kv_rows = None
        e._ids_host = None
        e._mix_host = None
        e.adapter_mix = None            # (its own table of mixes comes with the fork's own row buffers)
        e.row_sampling = None           # (allocated with the fork's own row buffers)
        if self.kv_scale is not None:
            e.kv_scale = self.kv_scale.clone()   # the scales belong to the engine's cache, not to the shared weights
        e._sink = torch.zeros(4, dtype=torch.int32, device=self.device)
        return e

    # ------------------------------------------------------------------------------------------------ buffers
    def _ensure(self, B: int, smax: int, paged=False, blocks=0, bs=16):
        """Buffers for B rows.  Contiguous cache: smax positions per row.  Paged cache: a pool of `blocks` blocks of `bs`
        positions (smax is then only the nominal window, nothing is sized by it)."""
        dev, T = self.device, self.dtype
        if B > self._cap_b:
            B = max(B, self._cap_b)
            self.h = torch.zeros(B, self.D, dtype=torch.float32, device=dev)
            Bp = nat.packed_rows(B)   # the packed layout works in 16-row tiles
            Kx = 0 if self.bank is None else self.bank.Kx   # adapter bank: the operands' shrink columns (k-steps at the end)
            self.q = torch.zeros(B, self.D, dtype=T, device=dev)
            if self.kv_dtype is not None:   # FP8 KV cache: the step's q | k | v rows, row-major (the attention launch appends k / v)
                self.qkv = torch.zeros(B, 3 * self.D, dtype=T, device=dev)
            self.a = torch.zeros(Bp, self.D + Kx, dtype=T, device=dev)
            self.f = torch.zeros(Bp, 4 * self.D + Kx, dtype=T, device=dev)
            self.xn = torch.zeros(Bp, self.D + Kx, dtype=T, device=dev)
            self.hb = torch.zeros(Bp, self.D, dtype=T, device=dev)   # "fold" mode: T-typed packed copy of the residual rows
            self.slab = torch.zeros(self.KSPLIT, B, self.D + 64, dtype=torch.float32, device=dev)   # + runtime-LoRA columns
            self.logits = torch.zeros(B, self.V, dtype=torch.float32, device=dev)
            self.tokens = torch.zeros(B, dtype=torch.int32, device=dev)
            self.finished = torch.zeros(B, dtype=torch.int32, device=dev)
            self.pad = torch.zeros(B, dtype=torch.int32, device=dev)
            self.force_stop = torch.full((B,), -1, dtype=torch.int32, device=dev)
            self.adapter_ids = torch.full((B,), -1, dtype=torch.int32, device=dev)   # adapter of each row (bank attached), -1 = base
            self.adapter_mix = self._mix_records([()] * B)                           # ... or its weighted mix of adapters (itts_lora_mix_row)
            self.row_step0 = torch.zeros(B, dtype=torch.int32, device=dev)   # loop step at which each row started (decode_refill)
            self.row_sampling = RowSampling(B, dev)                          # each row's own sampling settings (sp given as a list)
            self.kv_share = torch.zeros(1, dtype=torch.int32, device=dev)    # (p0 << 8) | C: rows' first C keys == row 0's at p0 (itts_attn_decode)
            self.state = torch.zeros(8, dtype=torch.int32, device=dev)
            self.history = torch.zeros(B, 2048, dtype=torch.int32, device=dev)
            self._cap_b = B
            self._cap_s = 0          # the contiguous cache follows the row buffers
            self._kv_pool = None
            self._graphs.clear()
        if paged:
            kv = self._kv_pool
            if kv is None or kv.rows < self._cap_b or kv.blocks < blocks or kv.bs != bs:
                kv = None
                self.kv = self._kv_pool = None          # release the old pool before the new one is allocated
                kv = self._kv_pool = PagedKV(self.L, self.H, self._cap_b, max(blocks, 2), bs,
                                             torch.uint8 if self.kv_dtype is not None else T, dev)
                self._graphs.clear()
            else:
                kv.reset()
            self.kv = kv
            self.kc, self.vc = kv.kc, kv.vc
            if self._cap_s:                              # a contiguous cache of an earlier (beam) batch: its graphs go with it
                self._cap_s = 0
                self._kc_rows = self._vc_rows = None
                self._graphs.clear()
            return
        self.kv = None
        if smax > self._cap_s:
            smax = (smax + 63) // 64 * 64
            if smax > 16384:
                raise ValueError(f"context {smax} exceeds the decode-attention limit of 16384 cache positions")
            self._kv_pool = None
            self._kc_rows = torch.zeros(self.L, self._cap_b, self.H, smax, 64, dtype=T, device=dev)
            self._vc_rows = torch.zeros(self.L, self._cap_b, self.H, smax, 64, dtype=T, device=dev)
            self._cap_s = smax
            self._graphs.clear()
        self.kc, self.vc = self._kc_rows, self._vc_rows

    def _kvargs(self):
        """Keyword arguments that tell a kernel where position j of a cache row lives."""
        return dict(kv_tab=self.kv.tab, kv_bs=self.kv.bs) if self.kv is not None else {}

    def export_kv(self, rows: int, S: int):
        """(K, V) [L, rows, H, S, 64] of cache positions [0, S) as VALUES: dense_kv() for a 16-bit cache; for the FP8 cache the
        decoded codes times their head's scale, fp32 (exact: an E4M3 value times a power of two)."""
        k, v = self.dense_kv(rows, S)
        if self.kv_dtype is None:
            return k, v
        sc = self.kv_scale[:, :, None, :, None, None]            # [L, 2, 1, H, 1, 1]
        return (quant.dequantize_kv(k, sc[:, 0]).to(torch.float32), quant.dequantize_kv(v, sc[:, 1]).to(torch.float32))

    # ------------------------------------------------------------------------------------------------ FP8 KV scales
    def set_kv_scales(self, scales):
        """scales [L][2][H] (K | V): positive powers of two, anything else is refused (the kernels and the host quantiser agree
        bit for bit because multiplying by the inverse is exact).  Device data: no captured step is invalidated."""
        if self.kv_dtype is None:
            raise ValueError("set_kv_scales(): the engine has no FP8 KV cache (kv_dtype='fp8')")
        t = torch.as_tensor(scales).detach().to("cpu", torch.float32)
        if tuple(t.shape) != (self.L, 2, self.H):
            raise ValueError(f"set_kv_scales(): expected shape [{self.L}, 2, {self.H}], got {list(t.shape)}")
        if not bool(quant.is_pow2(t).all()):
            raise ValueError("set_kv_scales(): every scale must be a positive power of two")
        self.kv_scale.copy_(t.to(self.device))

    def calibrate_kv_scales(self, prefix_emb: torch.Tensor, pad, headroom: float = 2.0):
        """Scales from one prompt batch: runs the ordinary un-shared prefill's layer loop over prefix_emb fp32 [B, P, D] (+ the start
        token), takes per layer and head the maximum of |k| and of |v| over the rows' real positions (torch on the layer's qkv
        buffer: off the hot path, one host sync) and writes quant.kv_scales_from_amax of those maxima.  Nothing is cached."""
        if self.kv_dtype is None:
            raise ValueError("calibrate_kv_scales(): the engine has no FP8 KV cache (kv_dtype='fp8')")
        B, P, D = prefix_emb.shape
        S, H, dev = P + 1, self.H, self.device
        pad_h = [int(v) for v in torch.as_tensor(pad).tolist()]
        if self._cap_b == 0:
            self._ensure(1, 64, paged=True, blocks=2)
        start = self.mel_emb[self.start_mel] + self.mel_pos[0]
        emb = torch.cat([prefix_emb.to(dev, torch.float32), start.expand(B, 1, D)], dim=1).contiguous()
        off = [0]
        for p in pad_h:
            off.append(off[-1] + S - p)
        idx = torch.cat([torch.arange(b * S + pad_h[b], (b + 1) * S) for b in range(B)])
        row_off = torch.tensor(off, dtype=torch.int32).to(dev)
        amax = torch.zeros(self.L, 2, H, dtype=torch.float32, device=dev)

        def attn(i, qkv, att):
            amax[i] = qkv.view(-1, 3, H, 64)[:, 1:].abs().amax(dim=(0, 3)).to(torch.float32)
            nat.attn_prefill_packed(qkv, att, None, None, row_off, None, B, S, H, 0)
        self._big_m_layers(emb.view(B * S, D)[idx.to(dev)], attn)
        self.kv_scale.copy_(quant.kv_scales_from_amax(amax.cpu(), headroom).to(dev))
        return self.kv_scale

    def dense_kv(self, rows: int, S: int):
        """(K, V) [L, rows, H, S, 64] of cache positions [0, S), in the cache's element type (T; uint8 codes for the FP8 cache, see
        export_kv): a dense copy whatever the cache layout (tests, tools)."""
        if self.kv is None:
            return self.kc[:, :rows, :, :S].clone(), self.vc[:, :rows, :, :S].clone()
        import numpy as np
        r, p = np.repeat(np.arange(rows), S), np.tile(np.arange(S), rows)
        blk, off = (torch.from_numpy(a).to(self.device) for a in self.kv.phys(r, p))
        k = self.kc[:, blk, :, off].view(rows, S, self.L, self.H, 64).permute(2, 0, 3, 1, 4).contiguous()
        v = self.vc[:, blk, :, off].view(rows, S, self.L, self.H, 64).permute(2, 0, 3, 1, 4).contiguous()
        return k, v

    # ------------------------------------------------------------------------------------------------ big-M passes
    def _proj_ksplit(self, M):
        """Split-K factor for the two N = D projections of a big-M pass: their 128 x 128 output tiles number M/128 x 10 -- 160 at the
        prefill's ~2 000 rows.  2-4 slices fill the chip (the factor is chosen below); the slabs are summed by the LayerNorm launch that
        follows (itts_ln_reduce: residual + bias + slabs, then LN), which replaces the GEMM's residual epilogue AND the LayerNorm
        launch.  1 where the tiles alone already fill the slots (the latent pass)."""
        if self.dtype == torch.float32 or self.D % 256 or os.environ.get("ITTS_PREFILL_KSPLIT", "1") == "0":
            return 1
        tiles = ((M + 127) // 128) * (self.D // 128)
        force = os.environ.get("ITTS_PREFILL_KS")          # measurement aid (tools/): a fixed factor
        if force:
            return max(1, int(force))
        if tiles > 270:
            return 1
        # a CU's share of the work, in whole-K tile units: ceil(tiles x ks / 256 CUs) slices of 1 / ks each (the kernel is priced by the
        # CU's load path, so two co-resident slices take twice one slice).  Config 3's prefill (M ~ 1 400: 110 tiles): ks = 2 -> 0.5
        # against 0.67 for ks = 3 (74 CUs would hold two slices) and 1.0 unsplit: 4.2 -> 3.8 ms; M ~ 2 000 (160 tiles): ks = 3 -> 0.67
        cus = 256
        cost = lambda ks: -(-tiles * ks // cus) / ks                                  # noqa: E731
        rule = 3 if tiles * 3 <= 540 else 2 if tiles * 2 <= 540 else 1               # round 3's choice (512 workgroup slots)
        best = min((1, 2, 3), key=lambda ks: (cost(ks), ks))
        return best if cost(best) < 0.9 * cost(rule) else rule

    def _big_m_layers(self, h, attn, row_ids=None, row_mix=None):
        """The 24 blocks over packed rows h fp32 [M, D] (in place): LayerNorm -> QKV -> attn(i, qkv, att) -> out-projection ->
        LayerNorm -> FC -> FC2.  With few rows the two N = D projections run split-K into slabs and the NEXT LayerNorm launch folds
        them into h (see _proj_ksplit); returns h with every block applied.
        With an adapter bank (row_ids int32 [M]: the adapter of every row, default -1) an adapted GEMM reads [x | u] row-major:
        x is copied into a [M, K + Kx] operand, itts_lora_shrink writes u behind it, and the GEMM runs with Cin = K + Kx over the
        extended weight -- one extra copy of the operand per adapted GEMM.  row_mix (uint8 [M, 32]: a mix record per row) in the
        place of row_ids: itts_lora_shrink_mix writes u."""
        T, D, dev = self.dtype, self.D, self.device
        M = h.shape[0]
        bank = self.bank
        if bank is not None:
            if row_ids is None and row_mix is None:
                row_ids = torch.full((M,), -1, dtype=torch.int32, device=dev)
            xc = {D: torch.empty(M, D + bank.Kx, dtype=T, device=dev), 4 * D: torch.empty(M, 4 * D + bank.Kx, dtype=T, device=dev)}

        def operand(l, wkey, x, K):
            """(packed weight, operand, Cin) of one GEMM of the block"""
            if bank is None or "bank_" + wkey not in l:
                return l.get(wkey + "_merged", l[wkey]), x, K
            c = xc[K]
            c[:, :K].copy_(x)
            nat.lora_shrink(x, None if row_mix is not None else row_ids, l["bank_a_" + wkey], c[:, K:], M, K, ldu=K + bank.Kx, mix=row_mix)
            return l["bank_" + wkey], c, K + bank.Kx
        xn = torch.empty(M, D, dtype=T, device=dev)
        qkv = torch.empty(M, 3 * D, dtype=T, device=dev)
        att = torch.empty(M, D, dtype=T, device=dev)
        ff = torch.empty(M, 4 * D, dtype=T, device=dev)
        ks = self._proj_ksplit(M)
        slab = torch.empty(ks, M, D, dtype=torch.float32, device=dev) if ks > 1 else None
        pending = None                       # bias of the projection whose slabs the next LayerNorm launch has to fold in
        for i, l in enumerate(self.layers):
            if pending is None:
                nat.layernorm(h, l["ln1"][0], l["ln1"][1], xn)
            else:
                nat.ln_reduce(h, l["ln1"][0], l["ln1"][1], xn, slab=slab, nslab=ks, bias=pending)
            w, x, K = operand(l, "w_qkv", xn, D)
            nat.gemm_conv(T, 1, M, M, K, 3 * D, w, x, qkv, bias=l["b_qkv"])
            attn(i, qkv, att)
            w, x, K = operand(l, "w_o", att, D)
            if ks > 1:
                nat.gemm_conv(T, 1, M, M, K, D, w, x, slab, y_f32=True, ksplit=ks)
                nat.ln_reduce(h, l["ln2"][0], l["ln2"][1], xn, slab=slab, nslab=ks, bias=l["b_o"])
            else:
                nat.gemm_conv(T, 1, M, M, K, D, w, x, h, bias=l["b_o"], y_f32=True, resid=h)
                nat.layernorm(h, l["ln2"][0], l["ln2"][1], xn)
            w, x, K = operand(l, "w_fc", xn, D)
            nat.gemm_conv(T, 1, M, M, K, 4 * D, w, x, ff, bias=l["b_fc"], act=1)
            w, x, K = operand(l, "w_pr", ff, 4 * D)
            if ks > 1:
                nat.gemm_conv(T, 1, M, M, K, D, w, x, slab, y_f32=True, ksplit=ks)
                pending = l["b_pr"]
            else:
                nat.gemm_conv(T, 1, M, M, K, D, w, x, h, bias=l["b_pr"], y_f32=True, resid=h)
        if pending is not None:              # the last block's FC2 slabs: fold them in (the LayerNorm output is not used)
            nat.ln_reduce(h, self.ln_f[0], self.ln_f[1], xn, slab=slab, nslab=ks, bias=pending)
        return h

    def _blocks_full(self, h, B, S, pad, use_cache, row_off=None, cache_shift=None, row_ids=None, row_mix=None):
        """All transformer blocks over h fp32 [M, D] (in place).  Padded form: M = B*S rows, pad int32 [B] (left padding)
        or None.  Packed form (row_off int32 [B+1] on device): only real rows exist, batch element b owns rows
        [row_off[b], row_off[b+1]), S is the longest element, cache row = cache_shift[b] + local row."""
        H = self.H
        kva = self._kvargs() if use_cache else {}

        def attn(i, qkv, att):
            kc, vc = (self.kc[i], self.vc[i]) if use_cache else (None, None)
            if use_cache and self.kv_dtype is not None:
                # FP8 cache: the attention runs without a cache (a form it has), one small launch quantises the layer's k / v
                nat.kv8_store(qkv, kc, vc, self.kv_scale[i], B, S, H, pad=pad, row_off=row_off, cache_shift=cache_shift, **kva)
                kc = vc = None
            if row_off is None:
                nat.attn_prefill(qkv, att, kc, vc, pad, B, S, H, self._cap_s)
            else:
                nat.attn_prefill_packed(qkv, att, kc, vc, row_off, cache_shift, B, S, H, self._cap_s, **({} if kc is None else kva))
        return self._big_m_layers(h, attn, row_ids, row_mix)

    def _head(self, h_rows, B):
        """ln_f -> final_norm -> mel_head on fp32 rows."""
        nat.ln_reduce(h_rows, self.ln_f[0], self.ln_f[1], self.xn, w2=self.final_norm[0], b2=self.final_norm[1], y_packed=self.pa)
        self._head_gemm(B, self.xn, self.logits)

    def _head_gemm(self, M, xn, logits):
        """mel_head over M normalised rows (fp32 logits); FP8 weights when the engine has them."""
        nat.gemm_skinny(self.dtype, M, self.V, self.D, self.w_head, self.b_head, x=xn, epi=nat.EPI_STORE_F32, yf=logits, x_packed=self.pa,
                        w_scale=self.s_head)

    def _prefill_shared(self, emb, pad_h, S, C):
        """The packed prefill pass for a batch whose elements all begin with the SAME C rows (one prompt's conditioning
        latents: no position embedding is added to them and they see only themselves, so their hidden states, keys and values
        are the same in every element).  Those C rows go through the blocks ONCE; every element contributes only its own rows
        (text + start token), whose attention reads the shared block's keys / values out of the same qkv buffer
        (itts_attn_prefill_shared: key tiles cut from sequence position 0 as in the un-shared pass, same bits per row).  The
        kernel appends every element's own rows to its cache row; the shared block's cache rows are copied to the other
        elements afterwards (itts_kv_share_rows: all layers in one launch).  Returns the hidden states of the elements' last rows."""
        import numpy as np
        T, D, H, dev = self.dtype, self.D, self.H, self.device
        B = emb.shape[0]
        own = [S - p - C for p in pad_h]                     # rows of each element behind the shared block
        if min(own) < 1:
            raise ValueError("prefill(shared_rows): an element has no row of its own behind the shared block")
        off = np.concatenate([[0, C], C + np.cumsum(own)]).astype(np.int64)
        M = int(off[-1])
        idx = np.concatenate([pad_h[0] + np.arange(C)] + [b * S + pad_h[b] + C + np.arange(own[b]) for b in range(B)])
        meta = torch.from_numpy(np.concatenate([
            idx, off, [0] + [C] * B, np.zeros(B + 1, np.int64), [0] + list(range(B)), [pad_h[0]] + [p + C for p in pad_h],
            off[2:] - 1]).astype(np.int64)).to(dev)                                                         # one upload
        E = B + 1
        o = 0

        def take(n, as32=True):
            nonlocal o
            t = meta[o:o + n]
            o += n
            return t.to(torch.int32) if as32 else t
        i_rows, row_off = take(M, False), take(E + 1)
        pre_len, pre_row0, w_row, w_pos0 = take(E), take(E), take(E), take(E)
        last_rows = take(B, False)
        h = emb.view(B * S, D)[i_rows]
        Smax = max(C, max(own))
        kva = self._kvargs()
        h = self._big_m_layers(h, lambda i, qkv, att: nat.attn_prefill_shared(
            qkv, att, self.kc[i], self.vc[i], row_off, pre_len, pre_row0, w_row, w_pos0, E, Smax, H, self._cap_s, **kva))
        if B > 1:   # the shared block's keys / values: cache row 0 -> the same sequence positions of every other cache row
            nat.kv_share_rows(self.kc, self.vc, B, H, C, pad_h[0], self.pad, self._cap_s, **self._kvargs())
        return h[last_rows].contiguous()

    def prefill(self, prefix_emb: torch.Tensor, pad: torch.Tensor, max_new: int, beams: int = 1, shared_rows: int = 0, paged=None,
                slots_window: int = 0, adapter_ids=None, adapter_mix=None):
        """prefix_emb fp32 [B,P,D] (left-padded with zeros), pad int [B].  Runs prefix + start token (mel position 0,
        model.py:152-162), fills the KV cache rows [pad_b, P] of every element, leaves logits of the last position in
        self.logits.  The left-padding rows are never computed: the real rows are packed (one gather), the GEMMs run over
        sum(P + 1 - pad_b) rows instead of B*(P+1), and the attention kernel writes each element's keys at its padded
        cache position, so the decode loop sees the reference's left-padded cache layout.
        shared_rows = C > 0: the caller promises that the first C real rows of every element are THE SAME rows (one prompt's
        conditioning latents, model.py:606-667 with a [1, C, D] conditioning tensor); they are then computed once for the
        batch (_prefill_shared: same logits and cache contents, a third fewer GEMM rows at config 3's shape).
        beams > 1 (beam search with the row table): HF expands every row to `beams` identical rows BEFORE the first forward;
        here the prompt is computed and cached ONCE per batch element (cache rows 0..B-1) and decode_beam() points the table
        entries of all its beams at that copy -- a third of the prefill work and prompt cache at 3 beams, identical values
        (the expanded rows are bit-wise copies).  The engine then holds B*beams rows: logits and pad are expanded here.
        paged (default: the engine's setting for beams == 1, never with beams > 1): the cache is a block pool behind a block
        table (class PagedKV).  Every row gets the blocks for its own window [pad_b, S + max_new]; a caller that goes on with
        decode_beam() over expanded rows passes paged=False (beam search addresses whole contiguous rows).  slots_window > 0
        (decode_refill's pool): size the pool for B rows of up to that many live positions each instead of this batch's.
        adapter_ids (host ints, one per element; needs attach_lora_bank): the adapter every row speaks with, -1 = the base voice;
        None with a bank attached = all base.  The ids reach the device as self.adapter_ids, which the decode step's shrink
        launches read: they are data, a captured step serves every assignment.
        adapter_mix (one mix per element, see check_adapter_mix; exclusive with adapter_ids): every row speaks with a weighted blend
        of up to four adapters.  The records reach the device as self.adapter_mix and the decode step's shrink launches become
        itts_lora_shrink_mix: that is structure (the graph key says which of the two launches a captured step holds), the
        records are data."""
        B, P, D = prefix_emb.shape
        S = P + 1
        beams = int(beams)
        ids, mix = self._voices(adapter_ids, adapter_mix, B)
        if self.kv_dtype is not None:
            if beams > 1:
                raise NotImplementedError("beam search over the FP8 KV cache (kv_dtype='fp8') is not built")
            if paged is not None and not paged:
                raise NotImplementedError("the FP8 KV cache (kv_dtype='fp8') is built for the paged cache only (paged=False)")
        if mix is not None and beams > 1:
            raise NotImplementedError("beam search with adapter mixes is not built")
        if ids is not None and beams > 1:
            raise NotImplementedError("beam search with an adapter bank is not built")
        if beams > 1 and self.beam_kv != "table":
            raise ValueError("prefill(beams>1) needs the KV row table (beam_kv='table')")
        pad_h = [int(v) for v in torch.as_tensor(pad).tolist()]
        # voice pool: the batch's voices become resident and stay pinned until the next prefill(); the device tables hold slots
        self._unpin_prefill()
        held = []
        s_ids, s_mix = self._slots(ids, mix, pin=held)
        self._prefill_pins = held
        use_pages = (self.paged if paged is None else bool(paged)) and beams == 1
        if use_pages:
            window = max(S + max_new + 1 - min(pad_h), int(slots_window))
            bs = 16 if window <= (KV_TAB - 2) * 16 else 32 if window <= (KV_TAB - 2) * 32 else 64
            if window > (KV_TAB - 2) * 64:
                use_pages = False      # a window no block table of 64 entries covers: contiguous rows
                if self.kv_dtype is not None:
                    raise NotImplementedError(f"the FP8 KV cache (kv_dtype='fp8') is built for the paged cache only: a window of "
                                              f"{window} positions does not fit the block table ({(KV_TAB - 2) * 64})")
        if use_pages:
            span = lambda lo, hi: ((hi - 1) // bs) - (lo // bs) + 1   # noqa: E731  blocks that cover positions [lo, hi)
            need = sum(span(p, S + max_new + 1) for p in pad_h)
            if slots_window:
                need = max(need, B * (int(slots_window) // bs + 2))
            self._ensure(B, S + max_new + 1, paged=True, blocks=need + 1, bs=bs)
            for b, p in enumerate(pad_h):
                self.kv.cover(b, p, S + max_new + 1)
            self.kv.flush()
        else:
            self._ensure(B * beams, S + max_new + 1)
        dev = self.device
        start = self.mel_emb[self.start_mel] + self.mel_pos[0]
        emb = torch.cat([prefix_emb.to(dev, torch.float32), start.expand(B, 1, D)], dim=1).contiguous()
        self._pad_host = pad_h             # latent_mel_rows() finds the prompt's K/V in the cache through it
        self.pad[:B] = torch.tensor(pad_h, dtype=torch.int32).to(dev)
        self.kv_share.zero_()
        self._ids_host, self._mix_host = ids, mix
        if ids is not None:
            self.adapter_ids[:B] = torch.tensor(s_ids, dtype=torch.int32).to(dev)
        if mix is not None:
            self.adapter_mix[:B] = self._mix_records(s_mix)
        # (with a bank the conditioning rows' hidden states depend on the row's adapter: nothing is shared)
        # (FP8 KV cache: the shared-prefix path is off in this version -- the un-shared prefill runs and kv_share stays 0)
        if shared_rows and B > 1 and self.share_prefix and ids is None and mix is None and self.kv_dtype is None:
            # every element starts with the same `shared_rows` rows (the caller's promise: one prompt's conditioning latents)
            self._head(self._prefill_shared(emb, pad_h, S, int(shared_rows)), B)
            if beams == 1 and int(shared_rows) <= 255 and self.share_kv_reads:
                # the decode attention reads those rows' keys / values from cache row 0 for every row (same bytes, one copy in L2)
                self.kv_share.fill_((pad_h[0] << 8) | int(shared_rows))
        else:
            lens = [S - p for p in pad_h]
            off = [0]
            for n in lens:
                off.append(off[-1] + n)
            idx = torch.cat([torch.arange(b * S + pad_h[b], (b + 1) * S) for b in range(B)])
            meta = torch.tensor(off + [b_off - 1 for b_off in off[1:]], dtype=torch.int32).to(dev)   # row_off | last rows
            row_off, last_rows = meta[: B + 1], meta[B + 1:].long()
            h = emb.view(B * S, D)[idx.to(dev)]
            h = self._blocks_full(h, B, S, None, True, row_off=row_off, cache_shift=self.pad[:B], **self._row_voices(s_ids, s_mix, lens))
            self._head(h[last_rows].contiguous(), B)
        self.state.zero_()                 # step, cache position, finished rows, arrival counter, seed (lo, hi)
        self.state[1] = S - 1
        self._pending_bump = False
        self.finished[:B] = 0
        self.row_step0.zero_()
        self.history[:B].zero_()
        self._B, self._S = B, S
        self._shared_prefix = None
        if beams > 1:
            R = B * beams
            self.logits[:R] = self.logits[:B].repeat_interleave(beams, dim=0)
            self.pad[:R] = self.pad[:B].repeat_interleave(beams)
            self._B = R
            self._shared_prefix = (B, beams)
        return self.logits[: self._B]

    def prefill_beams(self, prefix_emb, pad, max_new: int, beams: int, shared_rows: int = 0):
        """prefill() for decode_beam(): with the row table (beam_kv = "table") the prompt is computed and cached once per batch
        element; the copy form first expands every row to `beams` identical rows, as generate() does."""
        if self.kv_dtype is not None:
            raise NotImplementedError("beam search over the FP8 KV cache (kv_dtype='fp8') is not built")
        if self.beam_kv == "table":
            return self.prefill(prefix_emb, pad, max_new, beams=beams, shared_rows=shared_rows)
        return self.prefill(prefix_emb.repeat_interleave(beams, dim=0), pad.repeat_interleave(beams), max_new, shared_rows=shared_rows,
                            paged=False)

    def latent(self, emb: torch.Tensor, lengths=None, adapter_ids=None, adapter_mix=None) -> torch.Tensor:
        """Teacher-forced pass (model.py:459-474): emb fp32 [B,S,D] (right-padded rows allowed) ->
        final_norm(ln_f(blocks(emb))) fp32 [B,S,D].  With `lengths` (host ints, real rows per element) only the real rows
        are computed (packed); the padding rows of the result are zero.  adapter_ids / adapter_mix: as in prefill()."""
        B, S, D = emb.shape
        ids, mix = self._voices(adapter_ids, adapter_mix, B)
        if self._cap_b == 0:
            self._ensure(1, 64)
        dev = self.device
        src = emb.to(dev, torch.float32).contiguous().view(B * S, D)
        if lengths is None:
            h = src.clone()
            self._blocks_full(h, B, S, None, False, **self._row_voices(*self._slots(ids, mix), [S] * B))
            out = torch.empty_like(h)
            nat.layernorm(h, self.ln_f[0], self.ln_f[1], out, self.final_norm[0], self.final_norm[1])
            return out.view(B, S, D)
        lens = [int(n) for n in lengths]
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        idx = torch.cat([torch.arange(b * S, b * S + lens[b]) for b in range(B)]).to(dev)
        row_off = torch.tensor(off, dtype=torch.int32).to(dev)
        h = src[idx]
        self._blocks_full(h, B, max(lens), None, False, row_off=row_off, **self._row_voices(*self._slots(ids, mix), lens))
        packed = torch.empty_like(h)
        nat.layernorm(h, self.ln_f[0], self.ln_f[1], packed, self.final_norm[0], self.final_norm[1])
        out = torch.zeros(B * S, D, dtype=torch.float32, device=dev)
        out[idx] = packed
        return out.view(B, S, D)

    def latent_mel_rows(self, mel_emb: torch.Tensor, m_lens, cache_rows=None, adapter_ids=None, adapter_mix=None) -> torch.Tensor:
        """The teacher-forced pass (model.py:459-474, :548-597) over the MEL rows only, for the batch whose prompt the last
        prefill() cached.  In cond | text | mel the causal mask lets no prompt position see a mel position, so the prompt's
        keys and values in every layer are exactly what prefill() computed for the decode loop -- same kernels, same inputs,
        bit for bit -- and they are still in the KV cache at positions [pad_b, P) (the decode loop only appends behind them).
        Only the mel rows (start, codes, stop: ~60 % of the sequence) go through the GEMMs, LayerNorms and attention queries;
        the flash-attention kernel reads the prompt's K / V tiles from the cache rows and the mel rows' from this pass's qkv,
        with its key tiles cut from sequence position 0 as in latent().  Same bits as latent() on the whole sequence
        (tests/test_engines_gpu.py::test_latent_pass_reuses_the_cached_prompt).
        mel_emb fp32 [sum(m_lens), D]: the mel segments' embeddings, elements in prefill order; cache_rows: the cache row that
        holds element b's prompt (default b; b * num_beams after a beam prefill that copied rows; any subset of the prefilled rows,
        as the batched stream passes the rows that emit at a boundary).
        adapter_ids: the ids prefill() was given (the default), element b's that of its cache row: the cached prompt K / V were
        computed under them, other ids are refused.
        adapter_mix: likewise the mixes prefill() was given (the default after such a prefill); other mixes, or ids, are refused.
        Returns final_norm(ln_f(hidden)) fp32 [sum(m_lens), D]."""
        import numpy as np
        if self.kv_dtype is not None:
            raise NotImplementedError("latent_mel_rows(): the prompt-KV reuse reads the cache as T; over the FP8 KV cache "
                                      "(kv_dtype='fp8') run latent() on the whole sequence")
        T, D, H, dev = self.dtype, self.D, self.H, self.device
        B, P = len(m_lens), self._S - 1
        whole = cache_rows is None                         # the batch as prefilled: as many voices as rows
        cache_rows = list(range(B)) if whole else [int(r) for r in cache_rows]
        if len(cache_rows) != B or max(cache_rows) >= len(self._pad_host) or min(cache_rows) < 0:
            raise ValueError("latent_mel_rows(): the batch differs from the one prefill() cached")

        def cached(voices):      # the voices the prompts in cache_rows were prefilled under (None: none)
            if voices is None:
                return None
            if len(voices) != B if whole else max(cache_rows) >= len(voices):
                raise ValueError("latent_mel_rows(): the cached prompt was prefilled under other adapter ids" if voices is self._ids_host
                                 else "latent_mel_rows(): the cached prompt was prefilled under other adapter mixes")
            return [voices[r] for r in cache_rows]
        had_ids, had_mix = cached(self._ids_host), cached(self._mix_host)
        if adapter_ids is None and adapter_mix is None:
            ids, mix = had_ids, had_mix
        else:
            ids, mix = self._voices(adapter_ids, adapter_mix, B)
        if mix is not None and list(mix) != had_mix:
            raise ValueError("latent_mel_rows(): the cached prompt was prefilled under other adapter mixes")
        if ids is not None and list(ids) != had_ids:
            raise ValueError("latent_mel_rows(): the cached prompt was prefilled under other adapter ids")
        pads = [self._pad_host[r] for r in cache_rows]   # (a prefill of expanded beam rows lists the padding per cache row)
        pl = [P - p for p in pads]                        # real prompt rows per element
        m = [int(v) for v in m_lens]
        off = np.concatenate([[0], np.cumsum(m)])
        Mm = int(off[-1])
        if mel_emb.shape[0] != Mm:
            raise ValueError("latent_mel_rows(): mel_emb does not hold sum(m_lens) rows")
        meta = torch.from_numpy(np.concatenate([off, pl, cache_rows, pads]).astype(np.int32)).to(dev)   # one upload
        row_off, pre_len, pre_row, pre_pos0 = meta[: B + 1], meta[B + 1:2 * B + 1], meta[2 * B + 1:3 * B + 1], meta[3 * B + 1:]
        h = mel_emb.to(dev, torch.float32).contiguous()
        kva = self._kvargs()
        # the prompt's keys / values straight from the decode cache (itts_attn_prefill_prefix), the mel rows' from qkv
        h = self._big_m_layers(h, lambda i, qkv, att: nat.attn_prefill_prefix(
            qkv, att, self.kc[i], self.vc[i], row_off, pre_len, pre_row, pre_pos0, B, max(m), H, self._cap_s, **kva),
            **self._row_voices(*self._slots(ids, mix), m))
        out = torch.empty_like(h)
        nat.layernorm(h, self.ln_f[0], self.ln_f[1], out, self.final_norm[0], self.final_norm[1])
        return out

    # ------------------------------------------------------------------------------------------------ incremental latent pass
    LATENT_CACHE_BUDGET = 8 << 30      # bytes a latent_cache() may ask for (32 rows of 1 344 positions at 24 x 1280, 16-bit: 5.3 GB)

    def latent_cache(self, rows: int, cap: int) -> "LatentCache":
        """A K / V cache of the teacher-forced pass itself, for latent_append(): per layer the keys and values of every row
        the pass has computed, kc[l] / vc[l] of shape T [rows][H][cap][64] (T = the engine's dtype, also over an FP8 decode
        cache or FP8 weights), and the host array have[rows] -- the positions each row holds -- all zero.  cap is rounded up
        to a multiple of 64.  It belongs to a stream, not to the decode loop: nothing of the engine points at it.
        Size: layers x 2 x D x cap x itemsize per row (126 MB per row at 24 layers, D = 1280, cap = 1024, 16-bit).  A request
        above GPTEngine.LATENT_CACHE_BUDGET (8 GiB) is refused with ValueError before anything is allocated."""
        rows, cap = int(rows), int(cap)
        if rows < 1 or cap < 1:
            raise ValueError(f"latent_cache(): rows and cap must be at least 1 (got {rows}, {cap})")
        cap = (cap + 63) // 64 * 64
        need = LatentCache.nbytes(self.L, self.D, rows, cap, self.dtype)
        if need > self.LATENT_CACHE_BUDGET:
            raise ValueError(f"latent_cache(): {rows} rows of {cap} positions need {need} bytes, more than the budget of "
                             f"{self.LATENT_CACHE_BUDGET} (GPTEngine.LATENT_CACHE_BUDGET)")
        return LatentCache(self.L, self.H, rows, cap, self.dtype, self.device)

    def latent_append(self, cache: "LatentCache", emb: torch.Tensor, n_lens, cache_rows, adapter_ids=None, adapter_mix=None) -> torch.Tensor:
        """The teacher-forced pass (latent()) over the NEW rows of sequences whose earlier rows are in `cache`.
        emb fp32 [sum(n_lens), D]: element b's next n_lens[b] rows, which continue the sequence in cache row cache_rows[b] at
        position cache.have[cache_rows[b]].  The first call for a row carries its whole prompt cond | text followed by start |
        codes ...; later calls carry only the further mel rows.  The pass is causal, so what it returns for a row is final:
        final_norm(ln_f(hidden)) fp32 [sum(n_lens), D], the rows latent() gives for the same positions of the whole sequence
        (fp32: the same bits; 16-bit: the split-K factor of the projections follows the row count, see _proj_ksplit).
        Only the new rows go through the GEMMs, the LayerNorms and the attention queries; their keys and values are appended to
        the cache (itts_attn_prefill_shared, append form) and have advances.
        Refused with ValueError before anything is launched: have + n > cap, a cache row named twice, a cache of another engine
        shape, and voices (adapter_ids / adapter_mix, as latent() takes them) that differ from those the row's earlier rows were
        computed under -- the cache remembers them per row until reset().
        It allocates its operands, reads only weights and the latent cache and writes only the latent cache: none of the step's
        buffers, the decode cache or the refill staging buffers -- so it may run between two bursts of decode_chunks() /
        decode_refill_chunks() on the loop's stream, under the rule of decode_chunks."""
        import numpy as np
        B = len(n_lens)
        n = [int(v) for v in n_lens]
        rows = [int(r) for r in cache_rows]
        if B < 1 or len(rows) != B or min(n) < 1:
            raise ValueError("latent_append(): one cache row and at least one new row per element")
        if (cache.kc.shape[0], cache.kc.shape[2], cache.kc.dtype) != (self.L, self.H, self.dtype) or cache.kc.device != torch.device(self.device):
            raise ValueError("latent_append(): the cache was made for another engine (layers, heads, dtype or device differ)")
        if min(rows) < 0 or max(rows) >= cache.rows:
            raise ValueError(f"latent_append(): cache_rows must lie in [0, {cache.rows}): {rows}")
        if len(set(rows)) != B:
            raise ValueError(f"latent_append(): a cache row is named twice in one call: {rows}")
        have = [int(cache.have[r]) for r in rows]
        for r, h0, k in zip(rows, have, n):
            if h0 + k > cache.cap:
                raise ValueError(f"latent_append(): cache row {r} holds {h0} positions, {k} more do not fit its {cache.cap}")
        ids, mix = self._voices(adapter_ids, adapter_mix, B)
        voices = [("mix", mix[b]) if mix is not None else ("id", None if ids is None else ids[b]) for b in range(B)]
        for r, h0, v in zip(rows, have, voices):
            if h0 and cache.voice[r] != v:
                raise ValueError(f"latent_append(): cache row {r} was computed under another voice ({cache.voice[r]}, now {v})")
        if emb.dim() != 2 or emb.shape[0] != sum(n) or emb.shape[1] != self.D:
            raise ValueError("latent_append(): emb does not hold sum(n_lens) rows of D")
        if self._cap_b == 0:
            self._ensure(1, 64)
        dev, H = self.device, self.H
        off = np.concatenate([[0], np.cumsum(n)])
        meta = torch.from_numpy(np.concatenate([off, have, rows]).astype(np.int32)).to(dev)   # one upload
        row_off, pos0, w_row = meta[: B + 1], meta[B + 1:2 * B + 1], meta[2 * B + 1:]
        h = emb.to(dev, torch.float32).contiguous()
        if h is emb or h.data_ptr() == emb.data_ptr():
            h = h.clone()                                   # (the blocks run in place)
        h = self._big_m_layers(h, lambda i, qkv, att: nat.attn_prefill_append(
            qkv, att, cache.kc[i], cache.vc[i], row_off, pos0, w_row, pos0, B, max(n), H, cache.cap),
            **self._row_voices(*self._slots(ids, mix), n))
        out = torch.empty_like(h)
        nat.layernorm(h, self.ln_f[0], self.ln_f[1], out, self.final_norm[0], self.final_norm[1])
        for r, k, v in zip(rows, n, voices):
            cache.have[r] += k
            cache.voice[r] = v
        return out

    # ------------------------------------------------------------------------------------------------ decode loop
    def _sample(self, B, sp, dbg=None):
        """Token selection for all rows.  The loop state (step counter, cache position) is NOT advanced here: the next
        transformer step does it in its first LayerNorm launch (a launch that reads neither word), which takes a
        device-wide fence and a returning atomic per row out of the sampling kernel.  sp is PER_ROW: every row under its own
        record of the device table (itts_sample_rows)."""
        if sp is PER_ROW:
            nat.sample_rows(self.logits[:B], self.tokens, self.history, self.finished, self.state, self.extra_ids, self.force_stop,
                            self.row_sampling.tab, self.stop_mel, dbg, no_advance=True, row_step0=self.row_step0)
            self._pending_bump = True
            return
        nat.sample(self.logits[:B], self.tokens, self.history, self.finished, self.state, self.extra_ids, self.force_stop,
                   sp["repetition_penalty"], sp["temperature"], sp["top_k"], sp["top_p"], sp["do_sample"], sp["seed"],
                   self.stop_mel, dbg, no_advance=True, row_step0=self.row_step0)
        self._pending_bump = True

    def _fold_now(self, B):
        return self.decode_mode == "fold" and not self.lora and self.bank is None

    def _step_transformer(self, B, bump=None, gemm_only=False):
        """(bump: advance step counter / cache position inside this step's first launches; None = "a _sample call is
        waiting for it", which is what the token loop wants; the beam step kernel advances the state itself.)
        Transformer part of one cached decode step (model.py:163-193): embed token k at mel position k+1, 24 blocks,
        head.  "fold" form, 5 launches per block: QKV' (LayerNorm folded in, + K/V append) -> attention -> out-projection
        (+ residual update, T copy) -> FC' (folded, + gelu) -> FC2 (+ residual update, T copy); the loop state is advanced by
        launches that do not read the word they bump (embed_step: cache position; the first QKV': step counter).
        "launch" form, 7 per block: split-K slabs + [residual-reduce + LayerNorm] launches (itts_ln_reduce).
        gemm_only: ONLY the skinny GEMMs, with the step's real arguments; the loop state is left alone.  Returns (skinny-GEMM
        launches, algorithmic bytes: weights + input rows in T, and each epilogue's output)."""
        T, D, H, KS = self.dtype, self.D, self.H, self.KSPLIT
        es = T.itemsize
        step, pos = self.state[0:1], self.state[1:2]
        h, xn, pa = self.h[:B], self.xn, self.pa   # xn / a / f: whole buffers (packed layout is addressed from the base)
        if gemm_only:
            bump = False
        else:
            if bump is None:
                bump = getattr(self, "_pending_bump", False)
            self._pending_bump = False
        skip = lambda *a, **kw: None   # noqa: E731
        k = SimpleNamespace(embed_step=skip, attn_decode=skip, attn_decode_kv8=skip, ln_reduce=skip, lora_shrink=skip) if gemm_only else nat   # every other launch
        tally = [0, 0]

        def gemm(M, N, K, w, bias, epi, scale=None, **kw):
            """scale (fp32 [N]): w is a packed E4M3 image (weight_dtype "fp8"), one byte per weight."""
            nat.gemm_skinny(T, M, N, K, w, bias, epi=epi, w_scale=scale, **kw)
            out = {nat.EPI_QKV_CACHE: es, nat.EPI_STORE: es, nat.EPI_GELU_STORE: es, nat.EPI_RESID_F32: 2 * 4 + es,    # (h read and written, T copy)
                   nat.EPI_SLAB_F32: 4 * kw.get("ksplit", 1), nat.EPI_STORE_F32: 4}[epi]
            tally[0] += 1
            tally[1] += N * K * (es if scale is None else 1) + M * K * es + M * N * out
        w8 = self.weight_dtype == "fp8"
        rs0 = self.row_step0 if self._kv_rows is None else None
        kva = self._kvargs()
        attn_kw = dict(kv_rows=self._kv_rows, kv_step=step if self._kv_rows is not None else None,
                       skip_rows=self.finished if self._kv_rows is None and self.skip_finished else None,
                       kv_share=self.kv_share if self._kv_rows is None else None, **kva)
        if self._fold_now(B):
            hb = self.hb
            # mel position of token k is k + 1 (model.py:163-167); with a pending bump state[0] still holds k - 1
            k.embed_step(self.tokens, self.mel_emb, self.mel_pos, step, 2 if bump else 1, h, row_step0=rs0, h_packed=hb,
                         bump=pos if bump else None)
            r_o, r_p = self.fold_rows
            # more than 32 rows (beam search: 32 x 3): a workgroup that covers ALL rows moves 246 KB of activations through its
            # CU's load path per 1280-deep K; 32 rows per workgroup (the row tiles dealt to grid.z, 3-4 column tiles each so that
            # the grid still fits the chip) moves a third of that
            r_c = self.fold_rows_consumers if B > 32 else 0
            if B > 32:
                r_o, r_p = max(r_o, 32), max(r_p, 32)
            kv8 = self.kv_dtype is not None
            for i, l in enumerate(self.layers):
                qkv_kw = dict(x=hb, x_packed=True, ln_c=l["c_qkv"], bump=step if (bump and i == 0) else None, rows_per_wg=r_c, scale=l.get("s_qkv"))
                if kv8:
                    # FP8 KV cache: the existing row-major STORE epilogue writes q | k | v, and the attention launch quantises and
                    # appends the new key itself (still 5 launches per block); `bump` travels as before (it is not tied to an epilogue)
                    gemm(B, 3 * D, D, l["wf_qkv"], l["d_qkv"], nat.EPI_STORE, y=self.qkv, **qkv_kw)
                    k.attn_decode_kv8(self.qkv, self.kc[i], self.vc[i], self.a, self.pad, pos, self.kv_scale[i], B, H, out_packed=pa,
                                      skip_rows=attn_kw["skip_rows"], **kva)
                else:
                    gemm(B, 3 * D, D, l["wf_qkv"], l["d_qkv"], nat.EPI_QKV_CACHE, y=self.q, kcache=self.kc[i], vcache=self.vc[i],
                         pos=pos, heads=H, smax=self._cap_s, **qkv_kw, **kva)
                    k.attn_decode(self.q, self.kc[i], self.vc[i], self.a, self.pad, pos, B, H, self._cap_s, out_packed=pa, **attn_kw)
                gemm(B, D, D, l["w8_o" if w8 else "w_o"], l["b_o"], nat.EPI_RESID_F32, x=self.a, yf=h, y=hb, x_packed=pa, y_packed=True,
                     rows_per_wg=r_o, wide_wg=self.fold_wide, scale=l.get("s_o"))
                gemm(B, 4 * D, D, l["wf_fc"], l["d_fc"], nat.EPI_GELU_STORE, x=hb, y=self.f, x_packed=True, y_packed=pa,
                     ln_c=l["c_fc"], rows_per_wg=r_c, scale=l.get("s_fc"))
                gemm(B, D, 4 * D, l["w8_pr" if w8 else "w_pr"], l["b_pr"], nat.EPI_RESID_F32, x=self.f, yf=h, y=hb, x_packed=pa,
                     y_packed=True, rows_per_wg=r_p, wide_wg=self.fold_wide, scale=l.get("s_pr"))
            k.ln_reduce(h, self.ln_f[0], self.ln_f[1], xn, w2=self.final_norm[0], b2=self.final_norm[1], y_packed=pa)
        else:
            k.embed_step(self.tokens, self.mel_emb, self.mel_pos, step, 2 if bump else 1, h, row_step0=rs0)
            k.ln_reduce(h, self.layers[0]["ln1"][0], self.layers[0]["ln1"][1], xn, state_bump=self.state[0:2] if bump else None,
                        y_packed=pa)
            bank = self.bank
            Bp = nat.packed_rows(B)

            def adapted(l, wkey, x, K):
                """(packed weight, K) of one GEMM of the block.  Adapter bank: the rows' shrink vectors u = s_a x A_a^T go behind the
                operand's K / KS k-steps (the packed layout has the k-step outermost: the producers keep writing the front) and
                the GEMM runs over K + Kx with [W ; B_bank^T]."""
                if bank is None or "bank_" + wkey not in l:
                    return l.get(wkey + "_lora", l[wkey]), K
                mixed = self._mix_host is not None   # the batch was prefilled with adapter_mix: weighted slots from the rows' records
                k.lora_shrink(x, None if mixed else self.adapter_ids, l["bank_a_" + wkey], x.view(-1)[K * Bp:], B, K, x_packed=True,
                              u_packed=True, mix=self.adapter_mix if mixed else None)
                return l["bank_" + wkey], K + bank.Kx
            for i, l in enumerate(self.layers):
                last = i + 1 == self.L
                n_o = l.get("lora_n_o", D)
                n_p = l.get("lora_n_pr", D)
                w, K = adapted(l, "w_qkv", xn, D)
                gemm(B, 3 * D, K, w, l["b_qkv"], nat.EPI_QKV_CACHE, x=xn, y=self.q, kcache=self.kc[i], vcache=self.vc[i],
                     pos=pos, heads=H, smax=self._cap_s, x_packed=pa, **kva)
                k.attn_decode(self.q, self.kc[i], self.vc[i], self.a, self.pad, pos, B, H, self._cap_s, out_packed=pa, **attn_kw)
                nxt = self.ln_f if last else self.layers[i + 1]["ln1"]
                nxt2 = self.final_norm if last else (None, None)
                # out-projection: split-K slabs; with a runtime adapter the GEMM also produces x A in extra columns and the
                # reduce launch adds (x A) B^T
                sl_o = self.slab.view(-1)[: KS * B * n_o].view(KS, B, n_o)
                w, K = adapted(l, "w_o", self.a, D)
                gemm(B, n_o, K, w, None, nat.EPI_SLAB_F32, x=self.a, yf=sl_o, ksplit=KS, x_packed=pa)
                k.ln_reduce(h, l["ln2"][0], l["ln2"][1], xn, slab=sl_o, nslab=KS, bias=l["b_o"], y_packed=pa,
                            slab_stride=n_o, lora_b=l.get("lora_b_o"))
                w, K = adapted(l, "w_fc", xn, D)
                gemm(B, 4 * D, K, w, l["b_fc"], nat.EPI_GELU_STORE, x=xn, y=self.f, x_packed=pa, y_packed=pa)
                sl_p = self.slab.view(-1)[: KS * B * n_p].view(KS, B, n_p)
                w, K = adapted(l, "w_pr", self.f, 4 * D)
                gemm(B, n_p, K, w, None, nat.EPI_SLAB_F32, x=self.f, yf=sl_p, ksplit=KS, x_packed=pa)
                k.ln_reduce(h, nxt[0], nxt[1], xn, slab=sl_p, nslab=KS, bias=l["b_pr"], w2=nxt2[0], b2=nxt2[1], y_packed=pa,
                            slab_stride=n_p, lora_b=l.get("lora_b_pr"))
        gemm(B, self.V, D, self.w_head, self.b_head, nat.EPI_STORE_F32, x=self.xn, yf=self.logits, x_packed=pa, scale=self.s_head)
        return tuple(tally)

    def _poll(self):
        """One host synchronisation of the token loop: the number of finished rows."""
        return int(self.state[2].item())

    def _step_kernels(self, B, sp):
        self._step_transformer(B)
        self._sample(B, sp)

    def gemm_launches_of_step(self, B):
        """Measurement aid (bench.py): ONLY the skinny-GEMM launches of one decode step, with the step's real arguments
        (97 launches: 4 per block + the head).  Returns (GEMM launch count, algorithmic bytes); see _step_transformer."""
        return self._step_transformer(B, gemm_only=True)

    def _graph_key(self, kind, B, sp, nb=1):
        """Key of a captured decode step: the loop kind ("token" / "beam"), its rows and beams, the sampling parameters and
        every engine setting the captured launches read -- a setting changed after a capture must not replay the old variant."""
        key = (kind, B, nb, self.decode_mode, self.lora, tuple(self.fold_rows), self.fold_rows_consumers, self.fold_wide,
               self.pa, self.KSPLIT, self.skip_finished, self.share_kv_reads, self.beam_kv,
               None if self.kv is None else self.kv.bs, tuple(sorted(sp.items())), ("weights", self.weight_dtype),
               ("kv", self.kv_dtype))
        # an adapter bank: its shape and targets (what the captured launches were built from) -- never the rows' ids, which are data
        # ... nor their mixes; but WHICH shrink launch the step holds (ids or mix records) is structure
        if self.bank is None:
            return key
        return key + (("bank-mix" if self._mix_host is not None else "bank",) + self.bank.sig,)

    def _graph(self, key, body):
        """The CUDA graph of one decode step `body`, captured on first use and kept under `key` (see _graph_key)."""
        g = self._graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            with nat.CAPTURE_LOCK, torch.cuda.graph(g):  # no other thread may allocate / synchronise during a capture
                body()
            self._graphs[key] = g
        return g

    def _token_loop(self, n, stop, body, key, use_graph, check_every=0, rows=0, each=None):
        """Decode steps `body` from n tokens up to `stop`: the loop's first step (n = 1) runs eagerly and doubles as the
        warm-up, every later one replays the graph kept under `key` (eager throughout with use_graph False or force_eager).
        rows > 0: every check_every tokens the host polls, and the loop ends once all `rows` have finished.  each(): called
        after every step.  Returns the new token count."""
        graph = None
        while n < stop:
            if use_graph and not self.force_eager and n >= 2:
                if graph is None:
                    graph = self._graph(key, body)
                graph.replay()
            else:
                body()
            n += 1
            if each is not None:
                each()
            if rows and n % check_every == 0 and self._poll() >= rows:
                break
        return n

    @staticmethod
    def check_row_settings(rows, B, what="sp"):
        """A list of per-row sampling dicts (keys do_sample, temperature, top_k, top_p, repetition_penalty, seed, stream), checked
        on the host as the scalar form checks its arguments: ValueError before anything is launched."""
        if len(rows) != B:
            raise ValueError(f"{what} holds {len(rows)} rows of sampling settings for a batch of {B}")
        return [nat.check_sample_row(d, f"{what}[{b}]") for b, d in enumerate(rows)]

    def _rows_to_table(self, rows):
        """The loop runs under per-row settings: slot b <- rows[b] (checked), seeds in the records (state[4..5] = 0)."""
        self.state[4:6] = 0
        self.row_sampling.set(range(len(rows)), rows)
        self.row_sampling.flush()
        return PER_ROW

    def _loop_setup(self, who, max_new, sp, force_stop):
        """What the sampling loop needs after prefill(), for decode() and decode_chunks(): the checks, the cache cover, the
        force_stop upload.  Returns (B, sp checked, per_row); the caller seeds the state and draws token 1."""
        B = self._B
        per_row = isinstance(sp, (list, tuple))
        if per_row:
            sp = self.check_row_settings(sp, B)
        if self._shared_prefix is not None:
            raise ValueError(f"{who}(): prefill(beams=n) cached the prompt once per batch element; only decode_beam() can follow it")
        if self.kv is None and self._S + max_new + 1 > self._cap_s:
            raise ValueError(f"{who}(): max_new exceeds the capacity reserved by prefill()")
        if self.kv is not None:
            for b in range(B):                                   # (no-op when prefill() was given the same max_new)
                self.kv.cover(b, self._pad_host[b], self._S + max_new + 1)
            self.kv.flush()
        if force_stop is None:
            self.force_stop[:B] = -1
        else:
            self.force_stop[:B] = torch.as_tensor(force_stop, dtype=torch.int32).to(self.device)
        return B, sp, per_row

    def decode(self, max_new: int, sp, force_stop=None, use_graph=True, check_every=16, return_logits=False):
        """Run the sampling loop after prefill().  Returns codes int64 [B, n] padded with the stop token
        (HF generate semantics: rows that emitted EOS keep emitting pad = EOS).
        sp: one dict for the whole batch, or a list of B dicts (check_row_settings) -- every row under its own settings, seed and
        draw stream (itts_sample_rows); the captured step is the same for every such list."""
        B, sp, per_row = self._loop_setup("decode", max_new, sp, force_stop)
        logits_trace = [self.logits[:B].clone()] if return_logits else None
        sp = self._rows_to_table(sp) if per_row else self._seed_to_state(sp)
        self._sample(B, sp)  # token 1 from the prefill logits
        n = self._token_loop(1, max_new, lambda: self._step_kernels(B, sp), self._graph_key("token", B, sp), use_graph,
                             check_every, B, each=(lambda: logits_trace.append(self.logits[:B].clone())) if return_logits else None)
        self._poll()
        codes = self.history[:B, :n].to(torch.int64)
        return (codes, torch.stack(logits_trace, 0)) if return_logits else codes

    def decode_chunks(self, max_new: int, sp, chunk: int, force_stop=None, use_graph=True):
        """decode() as a generator: the sampling loop after prefill(), run in bursts of `chunk` tokens.  After every burst it polls
        and yields (codes int64 [B, n] on the host -- the n tokens every row has so far, stop-token padded as decode() pads --,
        finished flags bool [B] on the host); it ends when every row has finished or n == max_new.  Same set-up, same steps
        and the same graph key as decode(): one captured step serves both, and the tokens are decode()'s for the same sp.
        Between two bursts the caller may run latent_mel_rows() / latent() (and anything that is not the engine's) on the same
        stream: those passes work on buffers of their own (_big_m_layers allocates its operands, slabs included), read the
        prompt's cache positions only, and touch none of the step's h / hb / xn / a / f / q / slab / logits / state / tokens /
        history.  Not between bursts: prefill(), decode*() or anything else that writes the loop state."""
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("decode_chunks(): chunk must be at least one token")
        B, sp, per_row = self._loop_setup("decode_chunks", max_new, sp, force_stop)
        sp = self._rows_to_table(sp) if per_row else self._seed_to_state(sp)
        self._sample(B, sp)  # token 1 from the prefill logits
        key = self._graph_key("token", B, sp)
        body = lambda: self._step_kernels(B, sp)   # noqa: E731
        n = 1
        while True:
            # the next multiple of chunk (token 1, drawn from the prefill logits, counts towards the first burst)
            n = self._token_loop(n, min((n // chunk + 1) * chunk, max_new), body, key, use_graph)
            done = self._poll() >= B
            yield self.history[:B, :n].to(torch.int64).cpu(), self.finished[:B].cpu() != 0
            if done or n >= max_new:
                return

    # ------------------------------------------------------------------------------------------------ slot refill
    def _stage(self, rows, prefixes, stops, n, mixes=None):
        """Prepare new utterances for the decode slots `rows`, to JOIN a running loop at the moment every row has been given
        n tokens' worth of steps (state[0] = n - 1 with the bump pending, the next step writes cache position S+n-1).
        prefixes: fp32 [P_j, D] each (cond | text, no padding).  A new row is laid out exactly like an initial row of a batch
        whose loop started n - 1 steps later: prompt + start token at cache positions [pad, S+n-2] of its slot, left padding
        pad = S+n-1-(P_j+1).  One packed prefill pass over all new rows; their keys / values are kept aside ([M, L, H, 64]) and
        the logits of their last positions computed on buffers of their own -- nothing the running loop reads or writes is
        touched, so this may run on another stream beside the loop's steps.
        mixes (a loop with voices: one normalised mix per new row): the pass runs under the rows' records, which travel with the
        staged rows to the join, and so do int32 copies of the indices (what itts_refill_join reads)."""
        import numpy as np
        T, D, H, dev = self.dtype, self.D, self.H, self.device
        k = len(rows)
        end = self._S + n - 1                              # one past the last prompt position
        lens = [int(p.shape[0]) + 1 for p in prefixes]
        if max(lens) > end:
            raise ValueError("decode_refill(): a new prompt is longer than the positions the loop has passed")
        pads = [end - L for L in lens]
        start = (self.mel_emb[self.start_mel] + self.mel_pos[0])[None]
        h = torch.cat([t for p in prefixes for t in (p.to(dev, torch.float32), start)], dim=0).contiguous()
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        M = int(off[-1])
        slot = np.concatenate([np.full(L, r) for L, r in zip(lens, rows)])
        posi = np.concatenate([pd + np.arange(L) for L, pd in zip(lens, pads)])
        if self.kv is not None:                            # paged cache: (block, offset) of every staged position (the caller
            slot, posi = self.kv.phys(slot, posi)          # has dealt the new rows their blocks already)
        meta = torch.from_numpy(np.concatenate([slot, posi, off, off[1:] - 1, np.asarray(rows), np.asarray(pads),
                                                np.asarray(stops)]).astype(np.int64)).to(dev)     # one upload
        st = {"k": k, "n": n, "rows_h": list(rows), "i_b": meta[:M], "i_p": meta[M:2 * M],
              "i_rows": meta[2 * M + 2 * k + 1:2 * M + 3 * k + 1],
              "pads": meta[2 * M + 3 * k + 1:2 * M + 4 * k + 1].to(torch.int32), "stops": meta[2 * M + 4 * k + 1:].to(torch.int32)}
        row_off = meta[2 * M:2 * M + k + 1].to(torch.int32)
        last = meta[2 * M + k + 1:2 * M + 2 * k + 1]
        if mixes is not None:
            m32 = meta.to(torch.int32)
            st.update(mix=self._mix_records(mixes), i_b32=m32[:M], i_p32=m32[M:2 * M], rows32=m32[2 * M + 2 * k + 1:2 * M + 3 * k + 1])
        Tkv = T if self.kv_dtype is None else torch.uint8
        kst = torch.empty(M, self.L, H, 64, dtype=Tkv, device=dev)
        vst = torch.empty(M, self.L, H, 64, dtype=Tkv, device=dev)
        Smax = max(lens)

        def attn(i, qkv, att):     # keys / values are kept aside (they enter the cache when the rows join), plain causal attention
            q4 = qkv.view(M, 3, H, 64)
            if self.kv_dtype is not None:   # FP8 cache: the host quantiser, bit-equal to itts_kv8_store by construction
                kst[:, i] = quant.quantize_kv_e4m3(q4[:, 1], self.kv_scale[i, 0][None, :, None])
                vst[:, i] = quant.quantize_kv_e4m3(q4[:, 2], self.kv_scale[i, 1][None, :, None])
                nat.attn_prefill_packed(qkv, att, None, None, row_off, None, k, Smax, H, self._cap_s)
                return
            kst[:, i] = q4[:, 1]
            vst[:, i] = q4[:, 2]
            nat.attn_prefill_packed(qkv, att, None, None, row_off, None, k, Smax, H, self._cap_s)
        h = self._big_m_layers(h, attn, row_mix=None if mixes is None else self._row_mix(mixes, lens))
        xn_t = torch.zeros(nat.packed_rows(k), D, dtype=T, device=dev)
        lg_t = torch.empty(k, self.V, dtype=torch.float32, device=dev)
        nat.ln_reduce(h[last].contiguous(), self.ln_f[0], self.ln_f[1], xn_t, w2=self.final_norm[0], b2=self.final_norm[1],
                      y_packed=self.pa)
        self._head_gemm(k, xn_t, lg_t)
        st.update(kst=kst, vst=vst, logits=lg_t)
        return st

    def _join(self, st, sp, ev=None, row_sp=None, kernel=False):
        """The staged rows enter the loop (between two of its steps, at the n they were staged for): keys / values into the
        slots' cache rows, the first token of every new row sampled from its prefill logits -- on buffers of its own, the
        running rows' logits stay --, and the per-row state: left padding, stop step, own clock row_step0 = n - 1 (mel
        positions, history index and the repetition-penalty window count from the row's own first token).  ev: _stage ran
        on another stream and recorded it; the loop's stream waits for it and takes its buffers over.  row_sp (sp is PER_ROW): the
        new rows' own settings -- their first tokens are drawn under them and their slots' records written here, with row_step0.
        A loop with voices (st["mix"]: the new rows' records) also writes each entering slot's record into self.adapter_mix.
        kernel: everything behind the sample launch -- the two cache scatters, the row state, the voice records, state[2] -= k --
        is ONE launch (itts_refill_join); the torch form is kept as its oracle (decode_refill(join="torch"))."""
        k, n, dev = st["k"], st["n"], self.device
        kernel = kernel and "mix" in st
        if ev is not None:
            main = torch.cuda.current_stream(dev)
            main.wait_event(ev)
            for t in st.values():                       # allocated on the side stream, last used on this one
                if torch.is_tensor(t):
                    t.record_stream(main)
        if not kernel:
            self.kc[:, st["i_b"], :, st["i_p"]] = st["kst"]    # [M, L, H, 64] -> positions [pad, S+n-2] of the slots (rows | blocks)
            self.vc[:, st["i_b"], :, st["i_p"]] = st["vst"]
        tok_t = torch.zeros(k, dtype=torch.int32, device=dev)
        hist_t = torch.zeros(k, 8, dtype=torch.int32, device=dev)
        fin_t = torch.zeros(k, dtype=torch.int32, device=dev)
        step0_t = torch.full((k,), n - 1, dtype=torch.int32, device=dev)
        if not kernel:
            self.state[2:3] -= k                           # these slots were counted as finished
        if sp is PER_ROW:
            self.row_sampling.set(st["rows_h"], row_sp)
            self.row_sampling.flush()
            nat.sample_rows(st["logits"], tok_t, hist_t, fin_t, self.state, self.extra_ids, st["stops"],
                            self.row_sampling.tab[torch.tensor(st["rows_h"], device=dev)].contiguous(), self.stop_mel, None,
                            no_advance=True, row_step0=step0_t)
        else:
            nat.sample(st["logits"], tok_t, hist_t, fin_t, self.state, self.extra_ids, st["stops"], sp["repetition_penalty"],
                       sp["temperature"], sp["top_k"], sp["top_p"], sp["do_sample"], sp["seed"], self.stop_mel, None,
                       no_advance=True, row_step0=step0_t)
        if kernel:
            nat.refill_join(st["kst"], st["vst"], self.kc, self.vc, st["i_b32"], st["i_p32"], st["rows32"], tok_t, fin_t, st["stops"],
                            st["pads"], n - 1, self.tokens, self.history, self.finished, self.force_stop, self.row_step0, self.pad,
                            self.state, mix_new=st["mix"], mix=self.adapter_mix)
            return
        i_rows = st["i_rows"]
        self.tokens[i_rows] = tok_t
        self.history[i_rows, 0] = tok_t
        self.finished[i_rows] = fin_t
        self.force_stop[i_rows] = st["stops"]
        self.row_step0[i_rows] = step0_t
        self.pad[i_rows] = st["pads"]
        if "mix" in st:
            self.adapter_mix[i_rows] = st["mix"]

    def _stage_beside(self, side, fed, rows, prefixes, stops, n, mixes=None):
        """_stage on the stream `side` behind the event `fed`: (staged rows, the event that marks them ready)."""
        with torch.cuda.stream(side):
            side.wait_event(fed)
            for p in prefixes:
                p.record_stream(side)                   # allocated on the loop's stream, read on this one
            st = self._stage(rows, prefixes, stops, n, mixes)
            ev = torch.cuda.Event()
            ev.record(side)
        return st, ev

    refill_join = "kernel"      # decode_refill(join=None) of a loop with voices: the one-launch join (profiles/refill_voices.txt)

    @staticmethod
    def _fed_settings(item, sp_default):
        """The checked sampling settings of a fed item of a per-row loop: its own third element, else the loop's default."""
        own = item[2] if len(item) > 2 else None
        if own is None and sp_default is None:
            raise ValueError("decode_refill(): a fed item brings no sampling settings and no sp_default was given")
        return sp_default if own is None else nat.check_sample_row(own, "a fed item's settings")

    @staticmethod
    def _fed_voice(item):
        """The voice a fed item names -- its fourth element, (prefix, stop step, settings or None, voice): anything
        check_adapter_mix takes for one row.  The 2- and 3-tuples name none: the base voice."""
        return item[3] if len(item) > 3 else None

    def _poll_rows(self, owner, start, where, n, stopped_only=False):
        """The refill loop's poll after n steps, ONE record per slot that owns an utterance: {"utt": utterance id, "slot", "k": the
        row's own token count n - start[slot], "codes": history[slot, :k] (host int64; stop-token padded behind the row's stop),
        "stopped", "prompt": (cache row, first position, length) of the prompt's keys}.  One device-to-host copy of history[:B]
        (as wide as the longest live row) plus the flags.  The slots of the rows that have stopped become free and their blocks
        go back to the pool (the slot's later formal appends land in the scratch block).  stopped_only: only the rows that have
        stopped are copied and reported (a gather of those rows: what decode_refill has always read at a poll)."""
        self._poll()
        fin = self.finished[: len(owner)].tolist()
        live = [r for r, o in enumerate(owner) if o is not None and o >= 0 and (fin[r] or not stopped_only)]
        if not live:
            return []
        width = max(n - start[r] for r in live)
        if stopped_only:
            hist = dict(zip(live, self.history[torch.tensor(live, device=self.device), :width].cpu()))
        else:
            hist = self.history[: len(owner), :width].cpu()
        out = []
        for r in live:
            k = n - start[r]
            out.append({"utt": owner[r], "slot": r, "k": k, "codes": hist[r][:k].to(torch.int64), "stopped": bool(fin[r]),
                        "prompt": where[r]})
            if fin[r]:
                owner[r] = None
                if self.kv is not None:
                    self.kv.release(r)
        return out

    def decode_refill(self, max_new: int, sp, feed, force_stop=None, use_graph=True, check_every=16, positions=None,
                      staged=True, sp_default=None, voices=None, join=None, closed=None):
        """Continuous batching: the sampling loop after prefill(), with every slot whose row has emitted its stop token
        refilled from a queue (the mitigation for mixed output lengths).  num_beams = 1 only.
        feed(k) -> up to k items (prefix_emb fp32 [P, D] = cond | text without padding, stop step or -1); fewer than k means
        the queue is empty.  Rows are numbered in the order they entered: 0..B-1 = the prefilled batch, then the fed ones.
        max_new bounds every row's own length (a row that reaches it is stopped there).  Returns (codes, leftover): codes[id]
        int64 [n_id] ends with the stop token; leftover = items that were fed but could not be placed any more because the
        cache positions reserved by prefill() -- or the smaller budget `positions` -- ran out, or (paged cache) because a
        row's window no longer fits the block table or the free blocks (admit()); the caller starts a new loop with them.
        Every check_every steps the host reads the `finished` flags (the loop's one synchronisation).  staged = True: the
        prompts of the utterances that take the freed slots are prefilled on a SECOND STREAM while the loop runs its next
        check_every steps, and join at the following poll -- the ~300 launches of that pass are enqueued and executed under
        the loop's own steps instead of stalling it (the slot idles check_every steps longer).  staged = False: prefill and
        join at once, the loop waits.
        A row's tokens are those it would get decoded alone with the same logits (greedy: identical codes up to the usual
        reduction-order noise of a different left padding); sampled rows draw from the loop's Philox stream (row slot, loop
        step), so they differ from a stand-alone run as two seeds do.
        sp as a list of B dicts (check_row_settings): every row under its own settings.  A fed item may then carry its own dict as
        a third element, (prefix, stop step, settings); one that brings none gets sp_default.  The settings are written into the
        slot's record at the poll where the row enters; the row draws from (its seed, its stream, its own step), wherever and
        whenever it entered.
        voices (needs attach_lora_bank, and is needed with one): the prefilled rows' voices, one entry per row, each anything
        check_adapter_mix takes -- None / -1 (base), an id, {id: weight}, [(id, weight), ...]; they must be the voices the rows were
        prefilled under (prefill(adapter_mix=...) or adapter_ids=...).  A fed item names its voice as a fourth element,
        (prefix, stop step, settings or None, voice); an item without one speaks with the base voice.  Every voice is checked on
        the host, a fed item's at the poll where it is fed, before anything is launched for it.  The loop always runs the
        itts_lora_shrink_mix step (an id is the record {id, 1.0f}, bit-equal to the id launch): one captured graph serves the whole
        queue, whatever voices pass through a slot.  A row's record is written into self.adapter_mix[slot] when it joins; a freed
        slot gets the empty record at the poll that frees it.  join: "kernel" = the join is one launch behind the first-token
        sample (itts_refill_join), "torch" = the indexed writes it replaces, kept as its oracle; None = the engine's
        refill_join.  Loops without voices always run the torch form.
        closed: see decode_refill_chunks.  This call is that generator drained: one loop body serves both."""
        codes = {}
        for rec in self.decode_refill_chunks(max_new, sp, feed, force_stop=force_stop, use_graph=use_graph, check_every=check_every,
                                             positions=positions, staged=staged, sp_default=sp_default, voices=voices, join=join,
                                             closed=closed, records="stopped"):
            for row in rec["rows"]:
                if row["stopped"]:
                    c = row["codes"]
                    hit = (c == self.stop_mel).nonzero()
                    codes[row["utt"]] = c[: int(hit[0]) + 1] if hit.numel() else c
        return [codes[i] for i in range(len(codes))], self.refill_leftover

    def decode_refill_chunks(self, max_new: int, sp, feed, force_stop=None, use_graph=True, check_every=16, positions=None,
                             staged=True, sp_default=None, voices=None, join=None, closed=None, records="all"):
        """decode_refill() as a generator: the same arguments, checks, graph key ("token", B, sp), stages, join and refill_stats.
        At every poll -- the loop's one host synchronisation, every check_every steps: check_every is the chunk length -- it
        yields {"n": the loop's step count, "rows": one record per slot that owns an utterance (_poll_rows)}: the utterance id
        (entry order, as decode_refill numbers them), the slot, the row's own token count k = n - start[slot], its codes
        history[slot, :k] (host int64), whether it has stopped (a stopped row is reported once, at the poll that finds it; its
        slot is free from then on), and "prompt" = (cache row, first position, length): where the keys of its prompt (cond |
        text, without the start token) lie in the cache -- a caller may reuse them, or ignore them.  When the generator ends,
        self.refill_leftover holds what decode_refill returns as leftover.
        records = "stopped": a poll copies and reports only the rows that have stopped -- the gather decode_refill has always done
        at a poll, and what it (and infer_queue) drains this generator with: that path moves no more bytes than before.
        closed (a callable, or None): the explicit "no more will come" signal of an OPEN queue.  Without it (None) a feed that
        returns fewer than k items has said that the queue is empty, as ever.  With it, feed may return fewer than k items --
        none at all -- and is asked again at every later poll that finds a free slot, until closed() returns True behind such a
        short answer.  Either way the loop ends once no slot holds an utterance and the feed gave none at that poll: an idle
        loop is not kept spinning, the caller starts a new one when the next utterance arrives.
        Between two yields the caller may run latent() / latent_mel_rows() / the vocoder on the loop's stream, under the rule of
        decode_chunks.  A staged prefill (_stage_beside) may be running on the side stream at that time: it shares no buffer
        with those passes -- _stage and _big_m_layers allocate every operand per call (xn, qkv, att, ff, slabs, the bank's
        operands, kst / vst, the head's xn_t / lg_t), the passes read weights and, in latent_mel_rows, cache positions of
        prompts that have joined; the staged keys enter the cache only in _join, on the loop's stream, inside next().
        Closing the generator early abandons the loop: rows that were staged and have not joined are dropped (the loop's stream
        waits for the side stream's pass, so nothing of it is in flight when the next prefill() starts), the slots' blocks go
        back to the pool, and prefill() starts from a clean state as after any decode.
        The checks run, and the device work starts, with the first next()."""
        if records not in ("all", "stopped"):
            raise ValueError(f"decode_refill_chunks(): records must be 'all' or 'stopped' (got {records!r})")
        per_row = isinstance(sp, (list, tuple))
        if per_row:
            sp = self.check_row_settings(sp, self._B)
            if sp_default is not None:
                sp_default = nat.check_sample_row(sp_default, "sp_default")
        elif sp_default is not None:
            raise ValueError("decode_refill(): sp_default belongs to per-row settings (sp given as a list)")
        join = self.refill_join if join is None else join
        if join not in ("kernel", "torch"):
            raise ValueError(f"decode_refill(): join must be 'kernel' or 'torch' (got {join!r})")
        if self.bank is None and voices is not None:
            raise ValueError("decode_refill(): voices were given but no adapter bank is attached (attach_lora_bank)")
        if self.bank is not None and voices is None:
            raise NotImplementedError("decode_refill(): with an adapter bank attached the loop has to be told its rows' voices: "
                                      "voices=[...], one entry per prefilled row (None / -1 = the base voice, an id, or a mix), and "
                                      "a fed item's voice as its fourth element (prefix, stop step, settings or None, voice)")
        B, S, ce = self._B, self._S, int(check_every)
        if self._shared_prefix is not None or self._kv_rows is not None:
            raise ValueError("decode_refill(): num_beams = 1 only")
        voiced = voices is not None
        if voiced:
            mix = self.check_adapter_mix(voices, B, queue=True)    # (resident already: prefill() placed them)
            had = self._mix_host if self._mix_host is not None else [() if i < 0 else ((i, 1.0),) for i in self._ids_host or [-1] * B]
            if mix != list(had):
                raise ValueError("decode_refill(): voices differ from the voices the rows were prefilled under")
        kv = self.kv
        if kv is not None:
            # paged cache: the loop's position counter may grow for as long as the queue lasts -- a row only has to keep its own
            # window (prompt + max_new + the steps up to the poll that finds it stopped) inside the block table's ring
            limit = (1 << 30) if positions is None else int(positions)
            if max_new + 2 * ce + 2 > kv.window:
                raise ValueError("decode_refill(): max_new does not fit the block table's window")
        else:
            limit = self._cap_s if positions is None else min(self._cap_s, int(positions))
        if S + max_new + ce > limit:
            # the loop runs whole blocks of check_every steps before it looks at the flags again: the last rows can take
            # the loop check_every - 1 steps past max_new, and every step appends one K / V position for every slot
            raise ValueError("decode_refill(): the position budget must hold max_new + check_every positions behind the prompt "
                             "(prefill(max_new + check_every))")
        dev = self.device
        fs = [-1] * B if force_stop is None else [int(v) for v in force_stop]
        fs = [max_new - 1 if v < 0 else min(v, max_new - 1) for v in fs]
        self.force_stop[:B] = torch.tensor(fs, dtype=torch.int32).to(dev)
        sp = self._rows_to_table(sp) if per_row else self._seed_to_state(sp)
        pooled = voiced and self._pool() is not None
        res = self.bank.res if pooled else None
        row_pins = [[] for _ in range(B)]      # voice pool: the voices each slot's row holds a pin on
        unpin_next, held, guarded = [], [], []     # ... pins to drop when the loop is resumed; fed items that wait for a bank slot, their voices
        if voiced:      # from here on the step is the mix launch (graph key "bank-mix"), whichever launch the prefill ran
            self._ids_host, self._mix_host = None, mix
            if pooled:  # the rows take the pins over from prefill(): a row's voices are free again once it has left
                in_slots = self._slots(None, mix)[1]
                for b in range(B):
                    row_pins[b] = voice_pool.mix_voices(mix[b])
                    res.pin(row_pins[b])
                self._unpin_prefill()
            self.adapter_mix[:B] = self._mix_records(in_slots if pooled else mix)
            idle = self._mix_records([()])
        self.kv_share.zero_()                                # a refilled row 0 no longer holds the shared block where the others expect it
        owner, start = list(range(B)), [0] * B              # owner: utterance id | None (free) | -1 (reserved for staged rows)
        where = [(b, self._pad_host[b], S - 1 - self._pad_host[b]) for b in range(B)]   # the prompts' keys: (cache row, first position, length)
        ids, leftover, fed_out, pending, row_sp = itertools.count(B), [], False, None, None
        self.refill_leftover = leftover
        stats = self.refill_stats = {"steps": 0, "polls": 0, "refill_calls": 0, "rows_refilled": 0, "staged": bool(staged)}
        main = torch.cuda.current_stream(dev) if staged else None     # (only the staged form orders two streams)
        side = torch.cuda.Stream(device=dev) if staged else None
        if kv is not None:
            for b in range(B):      # the prefilled rows' whole windows, as admit() deals them (prefill(max_new + check_every) has)
                kv.cover(b, self._pad_host[b], S + max_new + ce)
            stats["blocks"], stats["peak_blocks"] = kv.blocks - 1, kv.used_blocks()
        step, key = (lambda: self._step_kernels(B, sp)), self._graph_key("token", B, sp)
        self._sample(B, sp)
        n = 1
        try:
            while True:
                if unpin_next:       # rows the last poll reported stopped: whatever the caller ran for them is enqueued by now
                    res.unpin(unpin_next)
                    unpin_next = []
                # ---- A: rows staged during the last steps join here
                if pending is not None:
                    st, ev, rows, row_sp = pending
                    self._join(st, sp, ev, row_sp, kernel=join == "kernel")
                    for r in rows:
                        owner[r], start[r] = next(ids), n - 1
                    pending = None
                # ---- B: utterances for the slots that are free now
                free = [r for r in range(B) if owner[r] is None]
                items = []
                if free and n > 1 and (held or not fed_out):
                    ask = max(0, len(free) - len(held))    # (items that wait for a bank slot go first: the order they were fed in)
                    items = list(feed(ask)) if ask and not fed_out else []
                    if len(items) > ask:
                        raise ValueError(f"decode_refill(): feed({ask}) returned {len(items)} items")
                    short = len(items) < ask
                    waited, items, held = len(held), held + items, []
                    fed_items = items    # (prefix, stop step[, settings[, voice]]) -> the old pairs + the rows' checked settings and voices
                    if per_row:
                        fed_sp = [self._fed_settings(it, sp_default) for it in items]
                    elif any(len(it) > 2 and it[2] is not None for it in items):
                        raise ValueError("decode_refill(): a fed item carries sampling settings but the loop runs under one dict "
                                         "(pass sp as a list)")
                    if voiced:
                        fed_mix = self.check_adapter_mix([self._fed_voice(it) for it in items], len(items), queue=True)
                    elif any(self._fed_voice(it) is not None for it in items):
                        raise ValueError("decode_refill(): a fed item names a voice but the loop runs without voices "
                                         "(attach_lora_bank, voices=[...])")
                    items = [tuple(it)[:2] for it in items]
                    # fewer than asked for: the queue is empty -- or, an open queue, only when closed() says so behind it
                    fed_out = fed_out or (short and (closed is None or bool(closed())))
                    if pooled:      # voice-aware admission: the first item whose voices find no slot, and every later one, wait
                        res.unguard(guarded)
                        fit = voice_pool.admit_voices(res, [voice_pool.mix_voices(m) for m in fed_mix])
                        self.bank.deferrals += len(items) - max(fit, waited)
                        held, items = fed_items[fit:], items[:fit]
                    n_join = n + ce if staged else n
                    placed = len(items)
                    if limit - (S + n_join + 1) < max_new + ce:     # steps the loop could still take
                        items = []
                    elif kv is not None:
                        items = items[:admit(kv, free, items, S + n_join - 1, max_new, ce)]
                    if len(items) < placed or (held and limit - (S + n_join + 1) < max_new + ce):
                        # not placed: as they were fed, settings and voice included -- and, behind them, those that waited for a voice
                        # (which this loop, out of positions, could never place either)
                        leftover[:] = fed_items[len(items):]
                        held = []
                    if pooled:      # a waiting item keeps its voices in the pool: remove() refuses them until it is placed or handed back
                        guarded = [v for m in fed_mix[fit: fit + len(held)] for v in voice_pool.mix_voices(m)]
                        res.guard(guarded)
                    fed_out = fed_out or bool(leftover)
                if items:
                    rows, prefixes = free[: len(items)], [p for p, _ in items]
                    row_sp = fed_sp[: len(items)] if per_row else None
                    row_mix = fed_mix[: len(items)] if voiced else None
                    if pooled:      # the new rows' voices: resident and paged in on this stream before `fed` is recorded, pinned
                        in_slots = self._slots(None, row_mix)[1]
                        for r, m in zip(rows, row_mix):
                            row_pins[r] = voice_pool.mix_voices(m)
                            res.pin(row_pins[r])
                        row_mix = in_slots
                    stops = [max_new - 1 if int(v) < 0 else min(int(v), max_new - 1) for _, v in items]
                    stats["refill_calls"] += 1
                    stats["rows_refilled"] += len(rows)
                    for r, pfx in zip(rows, prefixes):              # _stage lays the prompt + start token out in front of the join
                        where[r] = (r, S + n_join - 2 - int(pfx.shape[0]), int(pfx.shape[0]))
                    if not staged:
                        self._join(self._stage(rows, prefixes, stops, n, row_mix), sp, row_sp=row_sp, kernel=join == "kernel")
                        for r in rows:
                            owner[r], start[r] = next(ids), n - 1
                        items = []
                    else:
                        fed = torch.cuda.Event()
                        fed.record(main)                        # the prefix embeddings are complete on the loop's stream
                # no utterance in any slot and none fed: the end -- of a closed queue, and of an open one that has fallen idle
                if pending is None and not items and all(o is None for o in owner):
                    # no row holds a pin, and an item alone always fits the bank's slots: nothing can be waiting for a voice
                    assert not held, "decode_refill(): an item waits for a bank slot although no row is active"
                    if fed_out or closed is not None:
                        break
                # ---- C: check_every steps of the loop
                if kv is not None:
                    kv.flush()
                    stats["peak_blocks"] = max(stats["peak_blocks"], kv.used_blocks())
                if per_row:
                    self.row_sampling.flush()
                n = self._token_loop(n, n + ce, step, key, use_graph)
                # ---- D: the new rows' prompts, enqueued behind the steps on the host and run beside them on the GPU
                if items:
                    st, ev = self._stage_beside(side, fed, rows, prefixes, stops, n_join, row_mix)
                    pending = (st, ev, rows, row_sp)
                    for r in rows:
                        owner[r] = -1
                # ---- E: one host synchronisation: which rows have stopped -- and what every row has so far
                stats["steps"], stats["polls"] = n, stats["polls"] + 1
                record = self._poll_rows(owner, start, where, n, stopped_only=records == "stopped")
                freed = [row["slot"] for row in record if row["stopped"]]
                if voiced and freed:                            # an idle slot is the base voice (nothing reads what it computes)
                    self.adapter_mix[torch.tensor(freed, device=dev)] = idle
                for r in freed:
                    unpin_next.extend(row_pins[r])
                    row_pins[r] = []
                yield {"n": n, "rows": record}
        finally:
            if pending is not None:      # closed early: the staged rows never join; their pass ends before this stream goes on
                main.wait_event(pending[1])
                pending = None
            if pooled and self.bank is not None and self.bank.res is res:
                res.unpin(unpin_next + [v for pins in row_pins for v in pins])
                res.unguard(guarded)
            leftover.extend(held)        # (none when the loop ran to its end)
            if kv is not None:           # (all free already when the loop ran to its end)
                for r in range(B):
                    kv.release(r)

    # ------------------------------------------------------------------------------------------------ beam search
    def _ensure_beam(self, B: int, nb: int):
        R, dev = B * nb, self.device
        if getattr(self, "_beam_cap", (0, 0, 0)) == (B, nb, self._cap_s):
            return
        # the buffers below are about to be replaced: every captured beam step holds their addresses, so those graphs
        # must go with them (a B=4 -> B=3 -> B=4 sequence would otherwise replay a graph over freed memory)
        for key in [k for k in self._graphs if k and k[0] == "beam"]:
            del self._graphs[key]
        cap = self.history.shape[1]
        self.b_scores = torch.zeros(R, dtype=torch.float32, device=dev)
        self.b_src = torch.zeros(R, dtype=torch.int32, device=dev)
        self.b_hist = torch.zeros(2, R, cap, dtype=torch.int32, device=dev)
        self.b_hyp_score = torch.zeros(B, nb, dtype=torch.float32, device=dev)
        self.b_hyp_len = torch.zeros(B, nb, dtype=torch.int32, device=dev)
        self.b_hyp_tok = torch.zeros(B, nb, cap, dtype=torch.int32, device=dev)
        self.b_n_hyp = torch.zeros(B, dtype=torch.int32, device=dev)
        self.b_worst = torch.zeros(B, dtype=torch.float32, device=dev)
        self.b_done = torch.zeros(B, dtype=torch.int32, device=dev)
        self.b_kv_rows = torch.zeros(2, R, self._cap_s, dtype=torch.int32, device=dev)   # [parity][logical row][position]
        self.b_scratch = nat.beam_scratch(R, dev)   # per-row candidates handed from the step's first launch to its second
        self._beam_cap = (B, nb, self._cap_s)

    def _beam_select(self, B, nb, sp):
        R = B * nb
        self._pending_bump = False   # the beam step kernel advances step counter and cache position itself
        nat.beam_step(self.logits[:R], nb, self.tokens, self.b_src, self.b_scores, self.b_hist, self.b_hyp_score, self.b_hyp_len,
                      self.b_hyp_tok, self.b_n_hyp, self.b_worst, self.b_done, self.state, self.extra_ids,
                      sp["repetition_penalty"], sp["temperature"], sp["top_k"], sp["top_p"], sp["do_sample"],
                      sp.get("length_penalty", 0.0), sp["seed"], self.stop_mel, scratch=self.b_scratch)
        if self._kv_rows is not None:
            nat.beam_kv_rows(self._kv_rows, self.b_src, self.state)
        else:
            nat.beam_reorder_kv(self.kc, self.vc, self.b_src, self.state, B, nb)

    def _step_kernels_beam(self, B, nb, sp):
        self._step_transformer(B * nb)
        self._beam_select(B, nb, sp)

    def decode_beam(self, max_new: int, sp: dict, num_beams: int, use_graph=True, check_every=16, num_return_sequences=1):
        """Beam search / beam-sample after prefill() of B*num_beams rows (row = b*num_beams + beam, the beams of a batch
        element start as copies).  HF 4.44.2 semantics (oracle/beam_ref.py); returns int64 [B * num_return_sequences, n]: the
        num_return_sequences best hypotheses of every element, best first (row = b * num_return_sequences + rank),
        right-padded with the stop token."""
        nb = int(num_beams)
        if self.kv_dtype is not None:
            raise NotImplementedError("decode_beam(): beam search over the FP8 KV cache (kv_dtype='fp8') is not built")
        if self.bank is not None:
            raise NotImplementedError("decode_beam(): beam search with an adapter bank is not built")
        if isinstance(sp, (list, tuple)):
            raise NotImplementedError("decode_beam(): beam search with per-row sampling settings is not built")
        if not 1 <= int(num_return_sequences) <= nb:
            raise ValueError("num_return_sequences has to be in [1, num_beams]")   # generate() raises the same
        R = self._B
        if self.kv is not None:
            raise ValueError("decode_beam(): beam search addresses whole contiguous cache rows: prefill(..., paged=False) or prefill(beams=n)")
        if self._shared_prefix is not None and self._shared_prefix[1] != nb:
            raise ValueError("decode_beam(): prefill(beams=...) was given another beam count")
        assert R % nb == 0, "prefill() must have been given B*num_beams rows"
        B = R // nb
        if self._S + max_new + 1 > self._cap_s:
            raise ValueError("decode_beam(): max_new exceeds the capacity reserved by prefill()")
        self._ensure_beam(B, nb)
        self.kv_share.zero_()       # beam reorders (copy mode) move cache rows: the promise behind the shared reads does not hold
        self.b_scores.zero_()
        self.b_scores.view(B, nb)[:, 1:] = -1e9
        self.b_hist.zero_()
        self.b_n_hyp.zero_()
        self.b_worst.fill_(1e9)
        self.b_done.zero_()
        if self._shared_prefix is not None and self._shared_prefix != (B, nb):
            raise ValueError("decode_beam(): prefill(beams=...) was given another batch / beam count")
        if self.beam_kv == "table":
            rows = torch.arange(R, dtype=torch.int32, device=self.device)
            self.b_kv_rows[0] = rows[:, None]           # identity: every row holds itself ...
            if self._shared_prefix is not None:         # ... except the prompt, cached once per batch element in row b
                self.b_kv_rows[0][:, : self._S] = (rows // nb)[:, None]
            self._kv_rows = self.b_kv_rows
        else:
            self._kv_rows = None
        try:
            return self._decode_beam_loop(B, nb, max_new, sp, use_graph, check_every, int(num_return_sequences))
        finally:
            self._kv_rows = None

    def _decode_beam_loop(self, B, nb, max_new, sp, use_graph, check_every, num_return=1):
        sp = self._seed_to_state(sp)
        self._beam_select(B, nb, sp)  # token 1 from the prefill logits
        n = self._token_loop(1, max_new, lambda: self._step_kernels_beam(B, nb, sp), self._graph_key("beam", B * nb, sp, nb),
                             use_graph, check_every, B)
        self._poll()
        return self._beam_finalize(B, nb, n, float(sp.get("length_penalty", 0.0)), max_new, num_return)

    def _beam_finalize(self, B, nb, n, length_penalty, max_new, num_return=1):
        """BeamSearchScorer.finalize on the host: running beams of unfinished batch elements become hypotheses (score =
        sum_logprobs / generated_len**length_penalty), the num_return best hypotheses of each element are returned, best
        first (num_beam_hyps_to_keep = num_return_sequences; the device store already holds num_beams per element)."""
        hs = self.b_hyp_score.cpu().numpy()
        hl = self.b_hyp_len.cpu().numpy()
        ht = self.b_hyp_tok.cpu().numpy()
        nh = self.b_n_hyp.cpu().numpy()
        done = self.b_done.cpu().numpy()
        sc = self.b_scores.cpu().numpy().reshape(B, nb)
        hist = self.b_hist[n & 1].cpu().numpy().reshape(B, nb, -1)
        best = []
        for b in range(B):
            hyps = [(float(hs[b, i]), i, ht[b, i, : hl[b, i]].tolist()) for i in range(int(nh[b]))]
            if not done[b]:
                worst = min((h[0] for h in hyps), default=1e9)
                for k in range(nb):
                    score = float(sc[b, k]) / (float(n) ** length_penalty if length_penalty != 0.0 else 1.0)
                    if len(hyps) < nb or score > worst:
                        hyps.append((score, nb + k, hist[b, k, :n].tolist()))
                        if len(hyps) > nb:
                            hyps.remove(min(hyps, key=lambda h: (h[0], h[1])))
                        worst = min(h[0] for h in hyps)
            ranked = sorted(hyps, key=lambda h: (h[0], h[1]), reverse=True)
            best.extend(h[2] for h in ranked[:num_return])
        width = min(max(len(t) for t in best) + 1, max_new)  # sent_max_len = min(longest + 1, max_length)
        out = torch.full((len(best), width), self.stop_mel, dtype=torch.int64)
        for b, t in enumerate(best):
            out[b, : min(len(t), width)] = torch.tensor(t[:width], dtype=torch.int64)
        return out.to(self.device)

    def _seed_to_state(self, sp):
        """The draw key is launch-argument seed + state[4..5]; the loop keeps the argument at 0 and the real seed in the
        device state, so one captured step serves every seed (no re-capture per call)."""
        seed = int(sp.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
        lo, hi = seed & 0xFFFFFFFF, seed >> 32
        as_i32 = lambda v: v - (1 << 32) if v >= (1 << 31) else v  # noqa: E731
        self.state[4:6] = torch.tensor([as_i32(lo), as_i32(hi)], dtype=torch.int32).to(self.device)
        out = dict(sp)
        out["seed"] = 0
        return out

    def step_bytes(self, B: int, ctx: int) -> int:
        """Algorithmic HBM bytes of one decode step: weights once + KV read + KV append."""
        es = 1 if self.kv_dtype is not None else 4 if self.dtype == torch.float32 else 2   # bytes per cached element
        kv = self.L * 2 * self.D * es
        return self.weight_bytes + B * ctx * kv + B * kv
