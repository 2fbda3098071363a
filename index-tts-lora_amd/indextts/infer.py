"""IndexTTS inference orchestrator -- same Python surface as the reference's indextts/infer.py (class IndexTTS,
`infer`, `infer_fast`, `set_seed`), running the GPT decoder and the BigVGAN vocoder on hand-written gfx950 kernels.

Control flow follows the reference (infer.py:185-439 __init__, :446-497 remove_long_silence, :499-580 bucketing and
padding, :595-777 infer_fast, :779-917 infer); the arithmetic is in indextts.gpt.engine / indextts.BigVGAN.models.
Differences that are deliberate and visible: no CPU/MPS execution path (the HIP library is mandatory), bitsandbytes
quantisation and DeepSpeed are accepted in the config but not used, and the conditioning latents / speaker embedding of
a prompt are computed once per call instead of once per sentence (same values).
"""
from __future__ import annotations

import collections
import json
import os
import queue
import random
import threading
import time
import warnings
from typing import Dict, List

import numpy as np
import torch

from indextts import _native as nat
from indextts.BigVGAN.models import BigVGAN as Generator
from indextts.gpt.model import UnifiedVoice, row_sampling_params, sampling_params
from indextts.utils.audio import read_audio, write_pcm16, write_wav
from indextts.utils.pcm_out import OutputFormat, PcmOutEngine
from indextts.utils.post_wave import PostProcess, PostWaveEngine
from indextts.utils.tempo import SPEED_ONE, TempoEngine, fixed_speed
from indextts.utils.audio_engine import PromptAudioEngine, as_planar, refusal
from indextts.utils.checkpoint import load_checkpoint
from indextts.utils.config import Config, load_config
from indextts.utils.feature_extractors import MelSpectrogramFeatures, resample
from indextts.utils.front import TextNormalizer, TextTokenizer


def set_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _resolve_dtype(name):
    """The activation type of a precision name ("fp8": E4M3 weights under bf16 activations, see _resolve_gpt_precision)."""
    if name in ("bf16", "bfloat16"):
        return torch.bfloat16
    if name in ("fp16", "float16"):
        return torch.float16
    if name == "fp8":
        return torch.bfloat16
    return torch.float32


def _resolve_gpt_precision(gpt_p, quantization=None):
    """The `gpt` entry of a precision config -> (activation dtype, weight dtype: "fp8" | None, fell_back).  "fp8" is served: E4M3
    decode-step weights under bf16 activations.  The bitsandbytes formats (int8 / int4 / quantization.enabled) are not claimed: they
    fall back to bf16 weights, and fell_back says so."""
    quant = quantization or {}
    if quant.get("enabled", False) or gpt_p in ("int8", "int4"):
        return torch.bfloat16, None, True
    return _resolve_dtype(gpt_p), ("fp8" if gpt_p == "fp8" else None), False


def dedupe_prompts(cond_mel, n_rows, who="infer_batch"):
    """A prompt list (one [1, 100, T_i] mel per utterance) -> (the distinct prompts in the order they first appear, for every
    utterance the index of its prompt among them).  Two entries are the same prompt when they are the same tensor OBJECT: a
    service keeps one tensor per speaker, and comparing contents would cost a device pass per pair."""
    if len(cond_mel) != n_rows:
        raise ValueError(f"{who}: {len(cond_mel)} prompts for {n_rows} utterances (a prompt list names one prompt per utterance)")
    uniq, seen, idx = [], {}, []
    for m in cond_mel:
        if not torch.is_tensor(m) or m.dim() != 3 or m.shape[0] != 1:
            raise ValueError(f"{who}: every prompt of a list is a mel tensor [1, n_mels, T]")
        if id(m) not in seen:
            seen[id(m)] = len(uniq)
            uniq.append(m)
        idx.append(seen[id(m)])
    if len({int(m.shape[1]) for m in uniq}) != 1:
        raise ValueError(f"{who}: the prompts of a list have one number of mel bins")
    return uniq, idx


def _resolve_kv_cache(name):
    """The `kv_cache` entry of a precision config -> the engine's kv_dtype: "auto" (the default) = the activation type (None);
    "fp8" = one E4M3 byte per cached element (GPTEngine(kv_dtype="fp8")).  Any other value is an error."""
    if name is None or name == "auto":
        return None
    if name == "fp8":
        return "fp8"
    raise ValueError(f"precision_config: kv_cache must be 'auto' or 'fp8' (got {name!r})")


class _TextOrder:
    """Chunks of n rows that are produced interleaved, handed out in row order: what row i + 1 produces before row i has ended is
    held back (by reference) until then.  push(row, pcm, last) returns the chunks that may leave now."""

    def __init__(self, n):
        self.head, self.held, self.ended = 0, [[] for _ in range(n)], [False] * n

    def push(self, row, pcm, last):
        if pcm.numel():
            self.held[row].append(pcm)
        self.ended[row] = self.ended[row] or last
        out = []
        while self.head < len(self.held):       # head: the row whose chunks leave as they come
            out.extend(self.held[self.head])
            self.held[self.head] = []
            if not self.ended[self.head]:
                break
            self.head += 1
        return out

    def over(self):
        return self.head == len(self.held)


class _LatentRows:
    """What a stream with latent_cache=True keeps between two boundaries: the engine's latent cache (GPTEngine.latent_cache:
    the pass-2 keys / values of every row computed so far), and per cache row the mel rows it has been fed and the latents
    they gave (fp32 [frames, D], on the device).  A cache row is a stream's batch row, or a queue's decode slot."""

    def __init__(self, eng, rows, cap):
        self.cache = eng.latent_cache(rows, cap)
        self.fed, self.lat = [0] * rows, [None] * rows

    def reset(self, row):
        """The row's utterance has ended: its cache row starts the next one from position 0."""
        self.cache.reset(row)
        self.fed[row], self.lat[row] = 0, None


class _StreamState:
    """What a stream keeps between two boundaries, for IndexTTS._emit_boundary.  emitted: {utterance key: the frames it has given
    out} (an utterance not in it has given none, or has had its last event); left / right: the vocoder's halo; stop /
    max_mel_tokens: where a row ends; voice_kind: the keyword that names a voice to the latent pass (None: no voices); trace: the
    stream's _trace (or None), its "frames" / "latent" / "window" / "codes" indexed by an utterance's handle; latent: which pass
    a boundary runs -- "reuse" (repeated, over the prompt K / V the prefill left in the decode cache: _latents(reuse_prefix=True,
    cache_rows=...)), "whole" (repeated, the whole sequence) or a _LatentRows (incremental); warn: the words for a row that
    reaches max_mel_tokens, `{}` = its handle (None: nothing is said); out: a _StreamOut (the events carry the samples in its
    format) or None (fp32 at 24 kHz, as the vocoder leaves them)."""

    def __init__(self, halo, stop, max_mel_tokens, voice_kind, trace, latent, warn=None, out=None):
        self.emitted, (self.left, self.right), self.stop, self.max_mel_tokens = {}, halo, stop, max_mel_tokens
        self.voice_kind, self.trace, self.latent, self.warn, self.out = voice_kind, trace, latent, warn, out


class _StreamOut:
    """The output side of a stream whose caller named an OutputFormat: the PcmOutEngine, the format, and a PcmOutStream per
    utterance that has not had its last event (its carried filter tail, on the device)."""

    def __init__(self, engine, fmt):
        self.engine, self.fmt, self.streams = engine, fmt, {}

    def encode(self, rows):
        """rows: [(utterance key, fp32 pcm, last)] of ONE boundary -> their samples in the format, in one launch."""
        items = []
        for u, pcm, last in rows:
            s = self.streams.get(u)
            if s is None:
                s = self.streams[u] = self.engine.stream(self.fmt)
            items.append((s, pcm.to(torch.float32), last))
        outs = self.engine.push_many(items)
        for u, _, last in rows:
            if last:
                del self.streams[u]
        return outs


class IndexTTS:
    def __init__(self, cfg_path="checkpoints/config.yaml", model_dir="checkpoints", is_fp16=True, device=None,
                 use_cuda_kernel=None, speaker_info_path=None, precision_config=None, gpt_path=None,
                 prompt_frontend="torch", _weights=None, _cfg=None):
        if device is None:
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        if not str(device).startswith("cuda") or not torch.cuda.is_available():
            raise RuntimeError("this build of IndexTTS runs on an AMD GPU through libindextts_hip.so; "
                               f"device={device!r} is not supported (there is no CPU fallback)")
        if prompt_frontend not in ("torch", "hip"):
            raise ValueError(f"prompt_frontend must be 'torch' or 'hip' (got {prompt_frontend!r})")
        self.device = device
        self.is_fp16 = is_fp16
        self.use_cuda_kernel = True  # the fused HIP activation kernel is always used
        self.cfg = _cfg if _cfg is not None else load_config(cfg_path)
        self.model_dir = model_dir

        # precision: precision_config > config_inference.yaml > cfg.inference > is_fp16   (infer.py:213-304)
        source = "Runtime Args" if precision_config is not None else None
        if precision_config is None:
            p = os.path.join(model_dir, "config_inference.yaml") if model_dir else None
            if p and os.path.exists(p):
                icfg = load_config(p)
                if "inference" in icfg:
                    precision_config, source = icfg["inference"], "config_inference.yaml"
            elif "inference" in self.cfg:
                precision_config, source = self.cfg["inference"], "config.yaml [inference]"
        self.use_quantization = self.load_in_8bit = self.load_in_4bit = False
        self.gpt_weight_dtype = None     # "fp8": E4M3 decode-step weights (precision_config gpt: "fp8")
        self.kv_cache_dtype = None       # "fp8": E4M3 KV cache of the sampling loop (precision_config kv_cache: "fp8")
        if precision_config and isinstance(precision_config, dict):
            gpt_p = precision_config.get("gpt", "bf16")
            self.gpt_dtype, self.gpt_weight_dtype, fell_back = _resolve_gpt_precision(gpt_p, precision_config.get("quantization", {}))
            if fell_back:
                print(">> [warning] bitsandbytes quantisation is not available in this build; using BF16 weights")
            self.vocoder_dtype = _resolve_dtype(precision_config.get("vocoder", "bf16"))
            self.kv_cache_dtype = _resolve_kv_cache(precision_config.get("kv_cache", "auto"))
            gpt_s = "bf16 activations / e4m3 weights" if self.gpt_weight_dtype == "fp8" else str(self.gpt_dtype)
            kv_s = "e4m3" if self.kv_cache_dtype == "fp8" else "auto"
            print(f">> [config] mixed precision ({source}): GPT={gpt_s} kv_cache={kv_s} vocoder={self.vocoder_dtype}")
        elif self.is_fp16:
            self.gpt_dtype, self.vocoder_dtype = torch.bfloat16, torch.float32
            print(">> [config] BF16 GPT / FP32 vocoder (legacy is_fp16)")
        else:
            self.gpt_dtype = self.vocoder_dtype = torch.float32
            print(">> [config] FP32 (legacy)")
        if self.gpt_dtype == torch.float16:
            self.gpt_dtype = torch.bfloat16  # GPT kernels: fp32 | bf16
        self.dvae_dtype = self.gpt_dtype
        self.dtype = self.gpt_dtype if self.gpt_dtype != torch.float32 else None
        self.stop_mel_token = self.cfg.gpt.stop_mel_token

        if _weights is None:
            if gpt_path is not None:
                self.gpt_path = gpt_path if os.path.isabs(gpt_path) else os.path.join(model_dir, gpt_path)
            else:
                self.gpt_path = os.path.join(model_dir, self.cfg.gpt_checkpoint)
        else:
            self.gpt_path = None

        self._cache_conds = None
        self._feat_graphs = {}
        self._batch_feat = None   # (prompt tensor, its version counter, conds, spk) of the last infer_batch prompt
        self._batch_feat_rows = None   # the same of the last prompt LIST (_prompt_features_rows)
        # the latent pass takes the prompt's keys / values from the KV cache the decode loop leaves behind (same bits)
        self.reuse_prompt_kv = os.environ.get("ITTS_REUSE_PROMPT_KV", "1") == "1"
        self.gpt = UnifiedVoice(**self.cfg.gpt)
        if _weights is None:
            load_checkpoint(self.gpt, self.gpt_path)
        else:
            self.gpt.load_state_dict(_weights["gpt"])
        self.gpt = self.gpt.to(self.device).to(self.gpt_dtype).eval()
        self.gpt.post_init_gpt2_config(use_deepspeed=False, kv_cache=True, half=self.gpt_dtype != torch.float32,
                                       weight_dtype=self.gpt_weight_dtype, kv_dtype=self.kv_cache_dtype)
        print(f">> [system] GPT loaded ({self.gpt_dtype})")

        self.bigvgan = Generator(self.cfg.bigvgan, use_cuda_kernel=True)
        if _weights is None:
            self.bigvgan_path = os.path.join(model_dir, self.cfg.bigvgan_checkpoint)
            self.bigvgan.load_state_dict(torch.load(self.bigvgan_path, map_location="cpu")["generator"])
        else:
            self.bigvgan_path = None
            self.bigvgan.load_state_dict(_weights["bigvgan"])
        self.bigvgan = self.bigvgan.to(self.device).to(self.vocoder_dtype)
        self.bigvgan.remove_weight_norm()
        self.bigvgan.eval()
        print(f">> [system] BigVGAN loaded ({self.vocoder_dtype})")

        self.normalizer = TextNormalizer()
        self.normalizer.load()
        bpe = self.cfg.dataset["bpe_model"] if "dataset" in self.cfg else None
        self.bpe_path = os.path.join(model_dir, bpe) if (bpe and model_dir) else None
        self.tokenizer = TextTokenizer(self.bpe_path, self.normalizer, allow_synthetic=_weights is not None)

        self.cache_audio_prompt = None
        self.cache_cond_mel = None
        self._cache_spk = None
        self.gr_progress = None
        self.model_version = self.cfg.version if "version" in self.cfg else None
        self.speaker_list = []
        if speaker_info_path and os.path.exists(speaker_info_path):
            try:
                with open(speaker_info_path, "r", encoding="utf-8") as f:
                    self.speaker_list = [it["speaker"] for it in json.load(f) if "speaker" in it]
                print(f">> [system] multi-speaker mode ({len(self.speaker_list)} speakers)")
            except Exception as e:  # noqa: BLE001
                print(f">> [error] could not read speaker info: {e}")
        self.mel_extractor = MelSpectrogramFeatures()
        # "hip": wav -> log-mel on the device (utils/audio_engine.py); "torch" (default): the host ops above
        self.prompt_frontend = prompt_frontend
        self.audio_engine = PromptAudioEngine(self.device) if prompt_frontend == "hip" else None
        self._frontend_warned = False

    # `tts.gpt` is replaceable, as the reference's callers do when they hot-swap a fine-tuned checkpoint (api.py:118-175,
    # webui.py:107-160: build UnifiedVoice(**tts.cfg.gpt), load_checkpoint, .to / .eval / .half, post_init_gpt2_config, then
    # `tts.gpt = new_gpt; tts.gpt_path = path`).  Everything derived from the old weights goes with it: cached conditioning
    # latents and the captured conditioner graph.
    @property
    def gpt(self):
        return self._gpt

    @gpt.setter
    def gpt(self, module):
        self._gpt = module
        self._cache_conds = None
        self._feat_graphs = {}
        self._batch_feat = self._batch_feat_rows = None

    @gpt.deleter
    def gpt(self):   # `del tts.gpt` before the swap (api.py:160)
        self._gpt = None

    def reload_gpt(self, model_path: str):
        """The reference's model hot-swap (api.py:137-169) as one call: a new UnifiedVoice from `model_path` in this
        instance's precision replaces `self.gpt`.  Returns the config dict load_checkpoint found next to the file."""
        new_gpt = UnifiedVoice(**self.cfg.gpt)
        info = load_checkpoint(new_gpt, model_path)
        new_gpt = new_gpt.to(self.device).to(self.gpt_dtype).eval()
        new_gpt.post_init_gpt2_config(use_deepspeed=False, kv_cache=True, half=self.gpt_dtype != torch.float32,
                                       weight_dtype=self.gpt_weight_dtype, kv_dtype=self.kv_cache_dtype)
        del self.gpt
        self.torch_empty_cache()
        self.gpt = new_gpt
        self.gpt_path = model_path
        return info

    @classmethod
    def from_weights(cls, cfg, gpt_state_dict, bigvgan_state_dict, device="cuda:0", is_fp16=True, precision_config=None,
                     prompt_frontend="torch"):
        """Build from in-memory state dicts in the reference checkpoint key format (offline / synthetic weights)."""
        cfg = cfg if isinstance(cfg, Config) else Config(cfg)
        return cls(model_dir="", is_fp16=is_fp16, device=device, precision_config=precision_config, prompt_frontend=prompt_frontend, _cfg=cfg,
                   _weights={"gpt": gpt_state_dict, "bigvgan": bigvgan_state_dict})

    def replica(self) -> "IndexTTS":
        """Another instance over the same weight tensors (GPT packed weights, conditioner, vocoder) with its own KV cache,
        decode state, prompt caches and captured graphs -- for RequestPool."""
        import copy
        r = copy.copy(self)
        r.gpt = self.gpt.replica()
        r.cache_audio_prompt = r.cache_cond_mel = r._cache_conds = r._cache_spk = r._batch_feat = r._batch_feat_rows = None
        r._feat_graphs = {}       # captured graphs replay into their own static buffers: one set per instance
        return r

    # ------------------------------------------------------------------------------------------------ helpers
    def remove_long_silence(self, codes: torch.Tensor, silent_token=52, max_consecutive=30):
        """infer.py:446-497: cut at the first stop token; when a row holds more than `max_consecutive` silent tokens,
        keep at most 10 per run."""
        c, lens = IndexTTS._squeeze_silence_host(self, codes, silent_token, max_consecutive)   # (self: anything with stop_mel_token)
        return torch.from_numpy(c).to(codes.device), torch.tensor(lens, dtype=torch.long, device=codes.device)

    def _squeeze_silence_host(self, codes: torch.Tensor, silent_token=52, max_consecutive=30):
        """remove_long_silence on the host: (codes as a contiguous numpy array, lengths as a list) -- ONE device-to-host copy; the
        batch path keeps working from these host copies instead of uploading them and reading them back."""
        c = codes.detach().cpu().numpy()
        if c.shape[0] and not ((c == silent_token).sum(axis=1) > max_consecutive).any():
            # no row has a long silence (the usual case): only the cut at the first stop token, all rows at once
            is_stop = c == self.stop_mel_token
            lens = np.where(is_stop.any(axis=1), is_stop.argmax(axis=1), c.shape[1]).tolist()
            return np.ascontiguousarray(c[:, : max(lens)]), lens
        rows, lens, fixed = [], [], False
        for code in c:
            stops = np.nonzero(code == self.stop_mel_token)[0]
            n = int(stops[0]) if stops.size else code.shape[0]
            if int((code == silent_token).sum()) > max_consecutive:
                keep, run = [], 0
                for k in range(n):
                    if code[k] != silent_token:
                        keep.append(k)
                        run = 0
                    elif run < 10:
                        keep.append(k)
                        run += 1
                rows.append(code[keep])
                lens.append(len(keep))
                fixed = True
            else:
                rows.append(code[:n])
                lens.append(n)
        if fixed:
            if len(rows) > 1:
                m = max(len(r) for r in rows)
                out = np.full((len(rows), m), self.stop_mel_token, dtype=c.dtype)
                for i, r in enumerate(rows):
                    out[i, :len(r)] = r
                c = out
            else:
                c = rows[0][None]
        mx = max(lens)
        if mx < c.shape[1]:
            c = c[:, :mx]
        return np.ascontiguousarray(c), lens

    def bucket_sentences(self, sentences, bucket_max_size=4) -> List[List[Dict]]:
        """infer.py:499-550: sort by length, open a new bucket when a sentence is >= 1.5x the bucket median or the
        bucket is full, then fold singleton buckets into buckets with room."""
        items = [{"idx": i, "sent": s, "len": len(s)} for i, s in enumerate(sentences)]
        if len(items) <= bucket_max_size:
            return [items]
        buckets, last, median = [], None, 0
        for it in sorted(items, key=lambda x: x["len"]):
            if it["len"] == 0:
                continue
            if last is None or it["len"] >= int(median * 1.5) or len(last) >= bucket_max_size:
                last = [it]
                buckets.append(last)
                median = it["len"]
            else:
                last.append(it)
                median = last[len(last) // 2]["len"]
        out = [b for b in buckets if len(b) > 1]
        ones = [b[0] for b in buckets if len(b) == 1]
        if ones:
            for b in out:
                if len(b) < bucket_max_size:
                    b.append(ones.pop(0))
                    if not ones:
                        break
            if ones:
                out.extend([ones[i:i + bucket_max_size] for i in range(0, len(ones), bucket_max_size)])
        return out

    def pad_tokens_cat(self, tokens: List[torch.Tensor]) -> torch.Tensor:
        """infer.py:552-580: right-pad with the stop text token (v>=1.5), or 8 stops then start tokens (older)."""
        stop, start = self.cfg.gpt.stop_text_token, self.cfg.gpt.start_text_token
        if self.model_version and self.model_version >= 1.5:
            ts = [t.squeeze(0) for t in tokens]
            m = max(t.size(0) for t in ts)
            return torch.stack([torch.cat([t, torch.full((m - t.size(0),), stop, dtype=t.dtype, device=t.device)]) for t in ts])
        m = max(t.size(1) for t in tokens)
        outs = []
        for t in tokens:
            padn = m - t.size(1)
            if padn > 0:
                n = min(8, padn)
                t = torch.nn.functional.pad(t, (0, n), value=stop)
                t = torch.nn.functional.pad(t, (0, padn - n), value=start)
            outs.append(t[:, :m])
        return torch.cat(outs, dim=0)

    def torch_empty_cache(self):
        try:
            torch.cuda.empty_cache()
        except Exception:  # noqa: BLE001
            pass

    def _set_gr_progress(self, value, desc):
        if self.gr_progress is not None:
            self.gr_progress(value, desc=desc)

    def _prompt(self, audio_prompt):
        """infer.py:789-800: mono mean -> 24 kHz -> log-mel, cached by path; plus (new) cached conditioner outputs."""
        if self.cache_cond_mel is None or self.cache_audio_prompt != audio_prompt:
            self.cache_cond_mel = self._mels([self._decode(audio_prompt)])[0]
            self.cache_audio_prompt = audio_prompt
            self._cache_conds = self._cache_spk = None
        return self.cache_cond_mel

    @staticmethod
    def _decode(path):
        """A file -> (planar fp32 [C, N] on the host, its sample rate)."""
        audio, sr = read_audio(path)
        return torch.from_numpy(audio.T if audio.ndim > 1 else audio.reshape(1, -1)).float(), sr

    def _mel_torch(self, planar, sr):
        """The host front-end: mono mean -> 24 kHz -> log-mel in torch ops, then the upload."""
        audio = torch.mean(planar, dim=0, keepdim=True)
        audio = resample(audio, sr, 24000)
        return self.mel_extractor(audio).to(self.device)

    def _mels(self, decoded):
        """[(planar [C, N], sr), ..] -> their mels [1, 100, T_i] on the device.  prompt_frontend "hip": one pass of the audio
        engine over all of them; what the engine refuses (a rate whose tap table is too large, more than 8 channels, too few
        samples to reflect) goes through the torch path, with one warning per instance."""
        if self.audio_engine is None:
            return [self._mel_torch(p, sr) for p, sr in decoded]
        mels, take = [None] * len(decoded), []
        for i, (p, sr) in enumerate(decoded):
            why = refusal(tuple(p.shape), sr)
            if why is None:
                take.append(i)
                continue
            if not self._frontend_warned:
                self._frontend_warned = True
                warnings.warn(f"prompt_frontend='hip': {why}; such prompts go through the torch front-end", RuntimeWarning)
            mels[i] = self._mel_torch(p, sr)
        if take:
            for i, m in zip(take, self.audio_engine.mel([decoded[i][0] for i in take], [decoded[i][1] for i in take])):
                mels[i] = m
        return mels

    def prompt_mel(self, audio, sr=None):
        """The prompt mel [1, 100, T] (fp32, on the device) of a reference audio: what infer_batch, infer_queue, stream_batch,
        stream_queue and `more` take as cond_mel.  audio: a path, or an array / tensor [N] or [C, N] of decoded samples with its
        sample rate `sr`.  Runs the front-end this instance was built with (prompt_frontend); not cached."""
        return self.prompt_mels([audio], None if sr is None else [sr])[0]

    def prompt_mels(self, audios, srs=None):
        """prompt_mel of every entry of a list, in ONE pass of the audio engine under prompt_frontend="hip" (any rates, channel
        counts and lengths; every mel bit-equal to prompt_mel of that entry alone).  An entry is a path, an (array, sr) pair, or
        an array / tensor whose rate srs[i] gives."""
        decoded = []
        for i, a in enumerate(audios):
            if isinstance(a, (str, os.PathLike)):
                decoded.append(self._decode(a))
                continue
            if isinstance(a, tuple) and len(a) == 2:
                a, sr = a
            else:
                sr = None if srs is None else srs[i]
            if sr is None:
                raise ValueError("prompt_mel: decoded samples need their sample rate (sr)")
            decoded.append((as_planar(a), int(sr)))
        return self._mels(decoded)

    MAX_FEATURE_GRAPHS = 64     # (network, prompt shape) pairs kept captured: ~30 MB of activations + a graph each

    def _graphed(self, name, fn, cond_mel):
        """fn(prompt mel) through a CUDA graph per (network, prompt shape): the host-side PyTorch networks are a few hundred
        small launches each; the first call runs eagerly as warm-up, the second captures, later ones replay (any capture
        failure falls back to eager execution)."""
        key = (name,) + tuple(cond_mel.shape)
        ent = self._feat_graphs.get(key)
        if ent is None:
            if len(self._feat_graphs) >= self.MAX_FEATURE_GRAPHS:
                # a server that has seen this many prompt shapes starts over: the graphs go, and with them the per-length
                # activation buffers of the two front-end engines they replay into (this thread's)
                self._feat_graphs.clear()
                for eng in (self.gpt.conditioner(), self.bigvgan.speaker_engine()):
                    if eng is not None:
                        eng.forget()
            self._feat_graphs[key] = "warm"
            return fn(cond_mel)
        if ent == "warm":
            try:
                static_mel = cond_mel.clone()
                g = torch.cuda.CUDAGraph()
                with nat.CAPTURE_LOCK, torch.cuda.graph(g):
                    out = fn(static_mel)
                ent = (g, static_mel, out)
            except Exception as e:  # noqa: BLE001
                warnings.warn(f"prompt-feature graph capture failed ({e}); running eagerly", RuntimeWarning)
                ent = "eager"
            self._feat_graphs[key] = ent
        if ent == "eager":
            return fn(cond_mel)
        g, static_mel, out = ent
        static_mel.copy_(cond_mel)
        g.replay()
        return out.clone()

    def _prompt_conds(self, cond_mel):
        """Conditioning latents [1, 32, D] of a prompt mel (Conformer + Perceiver): all the first token needs."""
        return self._graphed("conds", lambda m: self.gpt.get_conditioning(m, None), cond_mel)   # None: rows are T frames long

    def _prompt_spk(self, cond_mel):
        """Speaker embedding [1, 1, 512] of a prompt mel (ECAPA-TDNN): only the vocoder needs it."""
        return self._graphed("spk", lambda m: self.bigvgan.speaker_embedding(m.transpose(1, 2)), cond_mel)

    def _prompt_features(self, cond_mel, spk=True):
        """(conditioning latents, speaker embedding) of a prompt mel, kept per prompt TENSOR: one prompt serves many batches
        (one speaker, a stream of texts), and the same object with an unchanged version counter is the same prompt, as infer()
        keeps them per prompt path (the cache holds a reference, so the storage cannot be recycled under it).  spk = False:
        the speaker embedding (ECAPA, vocoder input) is not on the first token's critical path; it is computed when first
        asked for and is None until then."""
        if isinstance(cond_mel, (list, tuple)):
            return self._prompt_features_rows(cond_mel, spk)
        bf = self._batch_feat
        if bf is None or bf[0] is not cond_mel or bf[1] != cond_mel._version:
            bf = self._batch_feat = [cond_mel, cond_mel._version, self._prompt_conds(cond_mel), None]
        if spk and bf[3] is None:
            bf[3] = self._prompt_spk(cond_mel)
        return bf[2], bf[3]

    def _prompt_features_rows(self, cond_mel, spk=True):
        """_prompt_features of a prompt list: (conds [B, 32, D], speaker embeddings [B, 1, 512]), row i those of utterance i's own
        prompt.  Every distinct prompt (dedupe_prompts) is conditioned once, each as if alone: a 16-bit model runs all of them
        through ONE pass of the HIP conditioner (ConditionerEngine.batch, run eagerly with a bounded buffer cache),
        fp32 loops the functional form; the speaker encoder runs once per distinct prompt.  Kept like the single prompt's
        features, per list of the same tensor objects at the same versions."""
        uniq, idx = dedupe_prompts(cond_mel, len(cond_mel))
        key = (tuple((id(m), m._version) for m in uniq), tuple(idx))
        bf = self._batch_feat_rows
        rows = torch.tensor(idx, device=self.device)
        if bf is None or bf[0] != key:
            ce = self.gpt.conditioner()
            if len(uniq) > 1 and ce is not None:
                # straight into the engine (the frames are copied once, into its concatenated mel); retain=False: no graph is
                # captured over this pass, so the engine keeps a bounded number of buffer sets however the batches are composed
                cu = ce.batch([m[0].to(self.device, torch.float32).t() for m in uniq], retain=False).clone()
            else:
                cu = torch.cat([self._prompt_conds(m) for m in uniq], 0)
            bf = self._batch_feat_rows = [key, uniq, cu[rows].contiguous(), None]     # (uniq: the ids in the key stay those tensors')
        if spk and bf[3] is None:
            bf[3] = torch.cat([self._prompt_spk(m) for m in uniq], 0)[rows].contiguous()
        return bf[2], bf[3]

    def _check_prompts(self, cond_mel, n_rows, gen, who):
        """A prompt list is checked before anything is launched; a list that names one prompt for every utterance IS that prompt
        (the single-tensor path, shared prefix and all)."""
        if not isinstance(cond_mel, (list, tuple)):
            return cond_mel
        uniq, _ = dedupe_prompts(cond_mel, n_rows, who)
        if int(gen.get("num_beams", 1)) > 1:
            raise NotImplementedError(f"{who}: beam search with a prompt per utterance is not built (num_beams = 1)")
        return uniq[0] if len(uniq) == 1 else list(cond_mel)

    def _conds(self, cond_mel, speaker_id=None):
        """Conditioning latents of the call.  The reference passes BOTH the prompt mel and speaker_ids=[speaker_id] to
        gpt.inference_speech / gpt.forward (infer.py:833-847, :864-874), and get_conditioning uses a stored
        mean_condition_{id} only when there is NO prompt mel (model.py:488-509): with an audio prompt -- which infer()
        always has -- the encoder path wins and speaker_id only has to be a known id.  Same here."""
        if cond_mel is None:
            return self.gpt.get_conditioning(None, None, speaker_ids=[speaker_id] if speaker_id else None)
        if self._cache_conds is None:
            self._cache_conds = self.gpt.get_conditioning(cond_mel, torch.tensor([cond_mel.shape[-1]], device=self.device))
        return self._cache_conds

    def _spk(self, cond_mel):
        if self._cache_spk is None:
            self._cache_spk = self.bigvgan.speaker_embedding(cond_mel.transpose(1, 2))
        return self._cache_spk

    def calibrate_kv(self, audio_prompt, text):
        """FP8 KV cache (precision_config kv_cache: "fp8"): choose the cache's scales from one prompt.  audio_prompt: a path (as
        infer()) or a prompt mel tensor (as infer_batch()); text: a string (split into sentences as infer() does) or a list of
        token-id rows.  Builds the prompt rows as infer does and runs GPTEngine.calibrate_kv_scales over them.  Until this is
        called every scale is 1.0.  Returns the scale table [L, 2, H]."""
        eng = self.gpt.engine
        if eng.kv_dtype is None:
            raise ValueError("calibrate_kv(): the KV cache is not FP8 (precision_config={'kv_cache': 'fp8'})")
        cond_mel = audio_prompt if torch.is_tensor(audio_prompt) else self._prompt(audio_prompt)
        if isinstance(text, str):
            sents = self.tokenizer.split_sentences(self.tokenizer.tokenize(text), 120)
            rows = [torch.tensor(self.tokenizer.convert_tokens_to_ids(sn), dtype=torch.int32) for sn in sents]
        else:
            rows = [torch.as_tensor(t).reshape(-1).to("cpu", torch.int32) for t in text]
        if not rows:
            raise ValueError("calibrate_kv(): no text rows")
        conds = self._prompt_features(cond_mel, spk=False)[0] if torch.is_tensor(audio_prompt) else self._conds(cond_mel)
        batch_h = torch.full((len(rows), max(int(t.numel()) for t in rows)), self.cfg.gpt.stop_text_token, dtype=torch.int32)
        for i, t in enumerate(rows):
            batch_h[i, : t.numel()] = t
        emb, pad = self.gpt.prefix_rows(conds, batch_h)
        return eng.calibrate_kv_scales(emb, pad)

    # ------------------------------------------------------------------------------------------------ voice pool
    def attach_voice_pool(self, voices=(), slots=32, rank=None):
        """Any number of LoRA voices behind `slots` bank slots (GPTEngine.attach_lora_pool).  voices:
        [(adapters, scaling), ...] in the attach_lora format; rank: the largest rank a voice of this pool may have (default: the
        largest among `voices`, 16 without any), padded to a multiple of 16; slots * padded rank <= 512.  Returns the voices' ids.
        From here on adapter_ids / adapter_mix of infer_batch, infer_queue, stream_batch, stream_queue and infer_stream name
        pool voice ids: a batch may name at most `slots` distinct voices (ValueError before anything is launched), a queue any
        number -- an utterance whose voices find no slot waits for one, and a loop runs as many decode slots as the leading utterances'
        voices fit the bank (`slots` of the queue calls may exceed the bank's).  Everything refused with a bank stays refused."""
        from indextts.gpt.voice_pool import VoicePool
        eng = self.gpt.engine
        voices = [(dict(ad), float(sc)) for ad, sc in voices]
        if rank is None:
            rank = max([int(A.shape[0]) for ad, _ in voices for A, _ in ad.values()] + [1])
        rank = int(rank)
        if not 1 <= rank <= 64:
            raise ValueError(f"attach_voice_pool(): rank must lie in [1, 64] (got {rank})")
        if eng.bank is not None:
            raise ValueError("attach_voice_pool(): an adapter bank or pool is attached (detach it first): one or the other")
        pool = VoicePool(eng, (rank + 15) // 16 * 16)
        ids = [pool.add(ad, sc) for ad, sc in voices]
        eng.attach_lora_pool(pool, slots)
        return ids

    def _voice_pool(self, who):
        pool = self.gpt.engine._pool()
        if pool is None:
            raise ValueError(f"{who}(): no voice pool is attached (attach_voice_pool)")
        return pool

    def add_voice(self, adapters, scaling) -> int:
        """One more voice for the attached pool, usable at once: no re-attach, no captured graph is dropped.  Returns its id."""
        return self._voice_pool("add_voice").add(adapters, scaling)

    def remove_voice(self, voice: int):
        """The voice leaves the pool (its id is never reused); ValueError while a batch or a queued utterance speaks with it."""
        self._voice_pool("remove_voice").remove(int(voice))

    # ------------------------------------------------------------------------------------------------ voices from checkpoints
    def voice_from_checkpoint(self, path_or_state_dict, return_report: bool = False, **kw):
        """(adapters, scaling) of the LoRA voice a MERGED fine-tuned checkpoint holds -- the one artifact the reference's train.py
        produces (gpt_finetuned.pth) -- against this instance's GPT weights as the base: GPTEngine.extract_lora (DESIGN.md section
        4.21).  A path goes through the checkpoint loader of utils/checkpoint.py; a state dict may be bare or wrapped as
        {'model': sd}.  kw: max_rank (16), gap (8.0), seed (0), ignore_other (False).  return_report: (adapters, scaling, report)
        with the rank and singular-value gap found per target.  ValueError for what is not a LoRA of this base."""
        from indextts.utils.checkpoint import _safe_load
        sd = _safe_load(path_or_state_dict) if isinstance(path_or_state_dict, (str, os.PathLike)) else path_or_state_dict
        adapters, scaling, report = self.gpt.engine.extract_lora(sd, **kw)     # (which takes the {'model': sd} wrapper off)
        return (adapters, scaling, report) if return_report else (adapters, scaling)

    def add_voice_from_checkpoint(self, path, **kw) -> int:
        """add_voice of voice_from_checkpoint(path, **kw): a merged fine-tuned checkpoint becomes a voice of the attached pool.
        Returns its id.  kw: max_rank, gap, seed, ignore_other (the report is voice_from_checkpoint's to return)."""
        self._voice_pool("add_voice_from_checkpoint")
        if "return_report" in kw:
            raise TypeError("add_voice_from_checkpoint() returns the pool id: ask voice_from_checkpoint(return_report=True) for the report")
        return self.add_voice(*self.voice_from_checkpoint(path, **kw))

    @staticmethod
    def save_voice(path, adapters, scaling):
        """A voice (adapters in the attach_lora format, scaling) as a file of tensors and a float only."""
        from indextts.gpt.voice_extract import save_voice
        save_voice(path, adapters, scaling)

    @staticmethod
    def load_voice(path):
        """(adapters, scaling) of a save_voice file, read with the weights-only unpickler."""
        from indextts.gpt.voice_extract import load_voice
        return load_voice(path)

    def detach_voice_pool(self):
        self._voice_pool("detach_voice_pool")
        self.gpt.engine.detach_lora_bank()

    @staticmethod
    def _gen_kwargs(kw):
        return dict(do_sample=kw.pop("do_sample", True), top_p=kw.pop("top_p", 0.8), top_k=kw.pop("top_k", 30),
                    temperature=kw.pop("temperature", 1.0), length_penalty=kw.pop("length_penalty", 0.0),
                    num_beams=kw.pop("num_beams", 3), repetition_penalty=kw.pop("repetition_penalty", 10.0)), \
            kw.pop("max_mel_tokens", 600)

    def _generate(self, conds, text_tokens, gen, max_mel_tokens, **extra):
        """gpt.inference_speech with precomputed conditioning latents (same values as recomputing them per call)."""
        g = self.gpt
        if g.engine.bank is not None:   # infer / infer_fast, the REST service's calls: no way to name a voice per request yet
            raise NotImplementedError("infer / infer_fast with an adapter bank is not built: use infer_batch(adapter_ids=...) or "
                                      "infer_batch(adapter_mix=...)")
        emb, pad = g.prefix_rows(conds, text_tokens)
        shared = int(conds.shape[1]) if conds.shape[0] == 1 else 0   # one prompt: every row starts with the same latents
        sp = sampling_params(gen, extra.pop("seed", torch.initial_seed() & 0x7FFFFFFFFFFFFFFF))
        nb = int(gen.get("num_beams", 1))
        if nb > 1:  # beam search / beam-sample: every row becomes num_beams rows (HF generate semantics)
            sp["length_penalty"] = float(gen.get("length_penalty", 0.0))
            g.engine.prefill(emb.repeat_interleave(nb, dim=0), pad.repeat_interleave(nb), max_mel_tokens, shared_rows=shared, paged=False)
            return g.engine.decode_beam(max_mel_tokens, sp, nb)
        g.engine.prefill(emb, pad, max_mel_tokens, shared_rows=shared)
        return g.engine.decode(max_mel_tokens, sp, force_stop=extra.pop("force_stop", None))

    def _latents(self, conds, text_rows: List[torch.Tensor], code_rows: List[torch.Tensor], reuse_prefix=False, cache_rows=None,
                 adapter_ids=None, adapter_mix=None, whole=False):
        """Teacher-forced pass for several utterances at once (right-padded; causal attention makes padding inert).
        Each row reproduces gpt(cond, text, [L], codes, code_len*1024, return_latent=True) of infer.py:864-874.
        The [cond | text | mel] embedding batch is assembled with two gathers from index arrays built on the host (one
        upload) instead of a dozen small launches per utterance.
        reuse_prefix: the rows are, in order, the batch the engine's LAST prefill() cached (same conds, same texts) and nothing
        has touched its KV cache since -- then only the mel rows are recomputed and the prompt's keys / values come from the
        cache (GPTEngine.latent_mel_rows: same bits, ~40 % fewer GEMM rows).
        adapter_ids: the rows' adapters of an attached bank (with reuse_prefix: the ids the cached prompt was prefilled under).
        adapter_mix: or the rows' mixes of adapters, under the same rule.
        whole: return (enc [B, S, D], nc) instead -- every real row of the pass, text rows included (score_codes); row b holds
        cond at 0 .. nc - 1, start_text | text | stop_text behind it, then start_mel | codes | stop_mel."""
        g, eng, dev = self.gpt, self.gpt.engine, self.device
        if conds.shape[0] not in (1, len(text_rows)):    # a subset of the rows with all rows' conds would speak in the wrong voices
            raise ValueError(f"_latents: conds holds {conds.shape[0]} prompts for {len(text_rows)} rows (one for all, or one per row)")
        if reuse_prefix and not whole and self.reuse_prompt_kv and eng.kv_dtype is None:   # (an FP8 cache holds codes: the prompt rows are recomputed)
            cl = [int(c.numel()) for c in code_rows]
            flat = torch.cat([c.reshape(-1).long() for c in code_rows]).cpu().numpy() if code_rows else np.zeros(0, np.int64)
            # start | codes | stop of every row and the position of each token in its row, for all rows at once
            cln = np.asarray(cl, dtype=np.int64)
            m = cln + 2
            offs = np.concatenate([[0], np.cumsum(m)])
            pos = np.arange(int(offs[-1])) - np.repeat(offs[:-1], m)
            ids = np.full(int(offs[-1]), g.stop_mel_token, dtype=np.int64)
            ids[pos == 0] = g.start_mel_token
            ids[(pos > 0) & (pos <= np.repeat(cln, m))] = flat
            idx = torch.from_numpy(np.stack([ids, pos])).to(dev)
            enc = eng.latent_mel_rows(eng.mel_emb[idx[0]] + eng.mel_pos[idx[1]], [c + 2 for c in cl], cache_rows,
                                      adapter_ids=adapter_ids, adapter_mix=adapter_mix)
            return [enc[int(offs[i]): int(offs[i]) + cl[i]] for i in range(len(cl))]

        def flat_host(rows):
            flat = torch.cat([r.reshape(-1).long() for r in rows]) if rows else torch.zeros(0, dtype=torch.long)
            return flat.cpu().numpy()

        tl = [int(t.numel()) for t in text_rows]
        cl = [int(c.numel()) for c in code_rows]
        tflat, cflat = flat_host(text_rows), flat_host(code_rows)
        nc = int(conds.shape[1])
        S = max(nc + t + 2 + c + 2 for t, c in zip(tl, cl))
        ri, ci, tok, pos, spans = ([], []), ([], []), ([], []), ([], []), []
        to = co = 0
        for i, (t, c) in enumerate(zip(tl, cl)):
            ti = np.concatenate([[g.start_text_token], tflat[to: to + t], [g.stop_text_token]])
            mi = np.concatenate([[g.start_mel_token], cflat[co: co + c], [g.stop_mel_token]])
            to, co = to + t, co + c
            for k, (ids, c0) in enumerate(((ti, nc), (mi, nc + ti.size))):
                ri[k].append(np.full(ids.size, i))
                ci[k].append(c0 + np.arange(ids.size))
                tok[k].append(ids)
                pos[k].append(np.arange(ids.size))
            spans.append((nc + ti.size, c))
        n_t = sum(a.size for a in tok[0])
        packed = np.stack([np.concatenate(ri[0] + ri[1]), np.concatenate(ci[0] + ci[1]), np.concatenate(tok[0] + tok[1]),
                           np.concatenate(pos[0] + pos[1])]).astype(np.int64)
        idx = torch.from_numpy(packed).to(dev)
        batch = torch.zeros(len(tl), S, conds.shape[2], dtype=torch.float32, device=dev)
        batch[:, :nc] = (conds if conds.shape[0] == len(tl) else conds[0]).to(dev, torch.float32)   # the row's own prompt, or the one
        batch[idx[0, :n_t], idx[1, :n_t]] = eng.text_emb[idx[2, :n_t]] + eng.text_pos[idx[3, :n_t]]
        batch[idx[0, n_t:], idx[1, n_t:]] = eng.mel_emb[idx[2, n_t:]] + eng.mel_pos[idx[3, n_t:]]
        enc = eng.latent(batch, lengths=[s0 + n + 2 for s0, n in spans], adapter_ids=adapter_ids, adapter_mix=adapter_mix)   # real rows only (cond | text | mel incl. start/stop)
        if whole:
            return enc, nc
        return [enc[i, s0: s0 + n] for i, (s0, n) in enumerate(spans)]

    def _latents_incremental(self, st: "_LatentRows", rows, conds, text_rows, code_rows, adapter_ids=None, adapter_mix=None):
        """_latents() for a stream that keeps a latent cache (st: _LatentRows; rows: the cache row of every element).  Only the
        part of each sequence the cache does not hold yet goes through the engine (GPTEngine.latent_append): on a row's first
        use its prompt rows cond | start_text text stop_text -- the index gather of _latents -- and then the mel rows start |
        codes[:k-1] beyond those already cached (the latent of frame t reads start and the codes < t: k rows give k frames).
        The latents a row has produced stay on the device (st.lat[row], fp32 [frames, D]: the vocoder's window reaches back
        into frames that were computed at earlier boundaries); returns, per element, its [k, D] latents."""
        g, eng, dev = self.gpt, self.gpt.engine, self.device
        if conds.shape[0] not in (1, len(text_rows)):
            raise ValueError(f"_latents: conds holds {conds.shape[0]} prompts for {len(text_rows)} rows (one for all, or one per row)")
        nc, D = int(conds.shape[1]), int(conds.shape[2])
        cl = [int(c.numel()) for c in code_rows]
        cflat = torch.cat([c.reshape(-1).long() for c in code_rows]).cpu().numpy() if code_rows else np.zeros(0, np.int64)
        c_dst, c_src, t_dst, t_tok, t_pos, m_dst, m_tok, m_pos = [], [], [], [], [], [], [], []
        sel, n_lens, mel0 = [], [], []          # the elements with new rows, their row counts, and where their mel rows start
        o = co = 0
        for i, (r, t, k) in enumerate(zip(rows, text_rows, cl)):
            fed, n = st.fed[r], 0
            codes, co = cflat[co: co + k], co + k
            if k > fed:
                if fed == 0:
                    ti = np.concatenate([[g.start_text_token], t.reshape(-1).numpy().astype(np.int64), [g.stop_text_token]])
                    c_dst.append(o + np.arange(nc))
                    c_src.append((i if conds.shape[0] > 1 else 0) * nc + np.arange(nc))
                    t_dst.append(o + nc + np.arange(ti.size))
                    t_tok.append(ti)
                    t_pos.append(np.arange(ti.size))
                    n = nc + ti.size
                mi = np.concatenate([[g.start_mel_token], codes[: k - 1]])[fed:k]
                m_dst.append(o + n + np.arange(mi.size))
                m_tok.append(mi)
                m_pos.append(fed + np.arange(mi.size))
                mel0.append(o + n)
                n += mi.size
                sel.append(i)
                n_lens.append(n)
                o += n
        if sel:
            cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)   # noqa: E731
            parts = [cat(c_dst), cat(c_src), cat(t_dst), cat(t_tok), cat(t_pos), cat(m_dst), cat(m_tok), cat(m_pos)]
            cut = np.cumsum([p.size for p in parts])
            idx = torch.from_numpy(np.concatenate(parts)).to(dev)                 # one upload
            cd, cs, td, tt, tp, md, mt, mp = (idx[a:b] for a, b in zip([0, *cut[:-1]], cut))
            emb = torch.empty(o, D, dtype=torch.float32, device=dev)
            if cd.numel():
                emb[cd] = conds.to(dev, torch.float32).reshape(-1, D)[cs]
                emb[td] = eng.text_emb[tt] + eng.text_pos[tp]
            emb[md] = eng.mel_emb[mt] + eng.mel_pos[mp]
            pick = lambda v: None if v is None else [v[i] for i in sel]           # noqa: E731
            enc = eng.latent_append(st.cache, emb, n_lens, [rows[i] for i in sel], adapter_ids=pick(adapter_ids),
                                    adapter_mix=pick(adapter_mix))
            for i, n, m0, off in zip(sel, n_lens, mel0, np.cumsum([0] + n_lens[:-1])):
                r, new = rows[i], enc[m0: off + n]
                st.lat[r] = new if st.lat[r] is None else torch.cat([st.lat[r], new], 0)
                st.fed[r] = cl[i]
        return [st.lat[r][:k] for r, k in zip(rows, cl)]

    # ------------------------------------------------------------------------------------------------ output formats
    def output_format(self, sample_rate=24000, encoding="pcm16") -> OutputFormat:
        """The value the `output=` keyword of the synthesis calls takes: the samples at `sample_rate` (any rate
        libindextts_out.so has a table for: 8000, 16000, 44100, 48000, ...) as "pcm16", "f32", "mulaw" or "alaw" (G.711), produced
        on the device (indextts/utils/pcm_out.py).  output=None, the default of every call, is what the calls have always
        returned: fp32 at 24 kHz in the int16 range (PCM16 in a file)."""
        return OutputFormat(sample_rate, encoding)

    @staticmethod
    def _check_output(output, who):
        if output is not None and not isinstance(output, OutputFormat):
            raise TypeError(f"{who}: output is an OutputFormat (IndexTTS.output_format(sample_rate, encoding)) or None")
        return output

    def _out_engine(self) -> PcmOutEngine:
        eng = getattr(self, "_pcm_out", None)
        if eng is None:
            eng = self._pcm_out = PcmOutEngine(self.device)
        return eng

    def _encode_rows(self, wavs, output):
        """Whole utterances (fp32 device tensors at 24 kHz) in the format `output`: one launch for all of them."""
        return self._out_engine().encode([w.reshape(-1).to(torch.float32) for w in wavs], output)

    # --------------------------------------------------------------------------------------------- waveform finishing
    def post_process(self, **kw) -> PostProcess:
        """The value the `post=` keyword of infer, infer_fast, infer_batch and infer_queue takes: trim_db, max_pause_ms, keep_ms,
        target_rms_db, peak_db (indextts/utils/post_wave.PostProcess) -- silence trimmed, pauses capped and the level set on the
        device, after the vocoder and before `output=`.  post=None, the default of every call, is what the calls have always
        returned.  The streams do not take it: a gain from whole-utterance statistics is not known at the first chunk."""
        return PostProcess(**kw)

    @staticmethod
    def _check_post(post, who):
        if post is not None and not isinstance(post, PostProcess):
            raise TypeError(f"{who}: post is a PostProcess (IndexTTS.post_process(trim_db=..., target_rms_db=..., ...)) or None")
        return post

    @staticmethod
    def _no_post(kw, who):
        if "post" in kw:        # (it would otherwise pass for a generation setting and be dropped unseen)
            raise TypeError(f"{who}: the streams do not take post= -- a gain from whole-utterance statistics is not known at the "
                            f"first chunk; use infer, infer_fast, infer_batch or infer_queue")

    def _post_engine(self) -> PostWaveEngine:
        eng = getattr(self, "_post_wave", None)
        if eng is None:
            eng = self._post_wave = PostWaveEngine(self.device)
        return eng

    def _post_rows(self, wavs, post):
        """Whole utterances (fp32 device tensors at 24 kHz) finished as `post` says: two launches for all of them."""
        return self._post_engine().process([w.reshape(-1).to(torch.float32) for w in wavs], post)

    # -------------------------------------------------------------------------------------------------- speaking rate
    @staticmethod
    def _check_speed(speed, who, n=None):
        """What the `speed=` keyword of infer, infer_fast, infer_batch and infer_queue asks for: None when nothing of the feature
        runs (speed None or 1.0, or every entry of a list one of the two), otherwise S = fixed_speed(speed) -- for a call of
        n utterances a list of n entries, S or None.  A bool, a value that is not finite or outside [0.5, 2.0], a list where one
        number is expected or a list of another length than n is a ValueError, raised before anything is launched."""
        if speed is None:
            return None
        try:
            if isinstance(speed, (list, tuple)):
                if n is None:
                    raise ValueError(f"speed = {speed!r}: one number for the call")
                if len(speed) != n:
                    raise ValueError(f"{len(speed)} speeds for {n} utterances")
                rows = [None if v is None else fixed_speed(v) for v in speed]
            else:
                rows = [fixed_speed(speed)] * (1 if n is None else n)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        if all(S is None or S == SPEED_ONE for S in rows):
            return None
        return rows[0] if n is None else rows

    @staticmethod
    def _check_pitch(pitch, speed, who, n=None):
        """What the `pitch=` keyword of infer, infer_fast, infer_batch and infer_queue asks for, beside the call's `speed=` as it
        was given (and already checked): None when nothing of the feature runs (pitch None or 0, or every entry of a list one of
        the two) -- the call then takes the speed= path exactly as it always has -- otherwise TempoEngine.plan(pitch, speed), for
        a call of n utterances a list of n of them (a row without a pitch keeps its speed).  More than 12 semitones either way,
        a speed / 2^(pitch / 12) outside [0.5, 2.0], a bool, a value that is not finite, a list where one number is expected or
        a list of another length than n is a ValueError, raised before anything is launched."""
        if pitch is None:
            return None
        try:
            if isinstance(pitch, (list, tuple)):
                if n is None:
                    raise ValueError(f"pitch = {pitch!r}: one number for the call")
                if len(pitch) != n:
                    raise ValueError(f"{len(pitch)} pitches for {n} utterances")
                pitches = list(pitch)
            else:
                pitches = [pitch] * (1 if n is None else n)
            speeds = list(speed) if isinstance(speed, (list, tuple)) else [speed] * len(pitches)
            plans = [TempoEngine.plan(p, s) for p, s in zip(pitches, speeds)]
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        if all(step is None for _, step in plans):
            return None
        return plans[0] if n is None else plans

    @staticmethod
    def _no_speed(kw, who):
        if "speed" in kw:       # (it would otherwise pass for a generation setting and be dropped unseen)
            raise TypeError(f"{who}: the streams do not take speed= -- the chain of lags is not carried across chunk boundaries; "
                            f"use infer, infer_fast, infer_batch or infer_queue")
        if "pitch" in kw:       # (pitch is WSOLA and a resampler behind it: the same chain)
            raise TypeError(f"{who}: the streams do not take pitch= -- the chain of lags is not carried across chunk boundaries; "
                            f"use infer, infer_fast, infer_batch or infer_queue")

    def _tempo_engine(self) -> TempoEngine:
        eng = getattr(self, "_tempo", None)
        if eng is None:
            eng = self._tempo = TempoEngine(self.device)
        return eng

    def _speed_rows(self, wavs, speeds):
        """Whole utterances (fp32 device tensors at 24 kHz) at the speeds S_i / 1024 (None: as it is): two launches for all of
        them; a row at None or 1024 comes back as the same tensor."""
        wavs = [w if w.dim() == 1 and w.dtype == torch.float32 else w.reshape(-1).to(torch.float32) for w in wavs]
        return self._tempo_engine().process(wavs, speeds)

    def _prosody_rows(self, wavs, speeds, plans):
        """_speed_rows when the call names no pitch (plans None); otherwise the rows at the pitch and speed of their
        TempoEngine.plan: three launches for all of them."""
        if plans is None:
            return self._speed_rows(wavs, speeds)
        wavs = [w if w.dim() == 1 and w.dtype == torch.float32 else w.reshape(-1).to(torch.float32) for w in wavs]
        return self._tempo_engine().shift_planned(wavs, plans)

    # ------------------------------------------------------------------------------------------------ audio -> codes
    def load_tokenizer(self, path=None, state_dict=None):
        """The acoustic tokenizer (indextts/vqvae/dvae.py): the DVAE's encoder and codebook from `path`, or
        from the config's dvae_checkpoint under model_dir, checked against the config's vqvae block -- or from a state dict
        in the reference's key format.  Nothing of it is loaded or imported until this is called (audio_codes and
        extract_codes call it).  Returns the CodecEngine."""
        from indextts.utils.checkpoint import check_dvae, load_dvae
        from indextts.vqvae.dvae import CodecEngine
        if state_dict is None:
            state_dict = load_dvae(self.cfg, self.model_dir, path)
        elif "vqvae" in self.cfg:
            check_dvae(state_dict, self.cfg["vqvae"])
        self._codec = CodecEngine(state_dict, self.device)
        return self._codec

    def _codec_engine(self):
        eng = getattr(self, "_codec", None)
        return eng if eng is not None else self.load_tokenizer()

    def audio_codes(self, audios, srs=None):
        """The mel codes of recordings: every entry (a path, an (array, sr) pair, or an array / tensor whose rate srs[i] gives, as
        prompt_mels takes them) through this instance's prompt front-end and the tokenizer, all clips in one ragged batch.
        Returns (codes, mels): int64 device tensors [code_count(T_i)] and the mels [1, 100, T_i] they were taken from."""
        eng = self._codec_engine()
        mels = self.prompt_mels(audios, srs)
        return eng.encode([m[0].to(torch.float32).contiguous() for m in mels]), mels

    def synthesize_codes(self, cond_mel, text_token_rows: List[torch.Tensor], code_rows: List[torch.Tensor], adapter_ids=None,
                         adapter_mix=None):
        """Copy synthesis: given codes -- of a recording (audio_codes), or what infer_batch(return_codes=True) returned -- through
        the teacher-forced latent pass and the vocoder of infer_batch, in the voice of cond_mel (one prompt, or a list with one
        per row) and under the rows' adapters.  Returns the fp32 waveforms, like infer_batch.  No token is sampled."""
        if len(code_rows) != len(text_token_rows):
            raise ValueError(f"synthesize_codes: {len(code_rows)} code rows for {len(text_token_rows)} texts")
        eng = self.gpt.engine
        if adapter_ids is not None:
            adapter_ids = eng._row_adapters(adapter_ids, len(text_token_rows))
        if adapter_mix is not None:
            adapter_mix = eng._voices(adapter_ids, adapter_mix, len(text_token_rows))[1]
        cond_mel = self._check_prompts(cond_mel, len(text_token_rows), {}, "synthesize_codes")
        conds, spk = self._prompt_features(cond_mel)
        rows = [c.reshape(-1).cpu().long() for c in code_rows]
        st = dict(conds=conds, spk=spk, rows=rows, texts=[t.reshape(-1).cpu() for t in text_token_rows], cache_rows=None,
                  cond_mel=cond_mel, adapter_ids=adapter_ids, adapter_mix=adapter_mix)
        return self._batch_waveforms(st, None, reuse_prefix=False)

    def extract_codes(self, audio_list, out_dir, batch_clips=16):
        """The first step of the fine-tuning workflow: the codes and mels of every clip of an audio list (one
        `path<TAB>transcript` per line; a relative path is relative to the list), in ragged batches of batch_clips.  Writes per
        clip <out_dir>/codes/<n>_<stem>.npy (int64 [1, T2]) and <out_dir>/mels/<n>_<stem>.npy (fp32 [1, 100, T]), as the
        reference's dataset loads them, and <out_dir>/metadata.jsonl with audio, text, codes, mels, duration per clip.
        Returns the metadata records."""
        base = os.path.dirname(os.path.abspath(audio_list))
        items = []
        with open(audio_list, "r", encoding="utf-8") as f:
            for n, line in enumerate(f):
                line = line.rstrip("\r\n")
                if not line.strip():
                    continue
                path, tab, text = line.partition("\t")
                if not tab or not path.strip():
                    raise ValueError(f"{audio_list}:{n + 1}: expected `path<TAB>transcript`")
                path = path.strip()
                items.append((path if os.path.isabs(path) else os.path.join(base, path), text.strip()))
        for sub in ("codes", "mels"):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        records = []
        for at in range(0, len(items), max(1, int(batch_clips))):
            chunk = items[at: at + max(1, int(batch_clips))]
            decoded = [self._decode(p) for p, _ in chunk]
            codes, mels = self.audio_codes([(d[0], d[1]) for d in decoded])
            for k, ((path, text), (planar, sr), c, m) in enumerate(zip(chunk, decoded, codes, mels)):
                name = f"{at + k:06d}_{os.path.splitext(os.path.basename(path))[0]}.npy"
                rec = dict(audio=path, text=text, codes=os.path.join(out_dir, "codes", name), mels=os.path.join(out_dir, "mels", name),
                           duration=float(planar.shape[-1]) / float(sr))
                np.save(rec["codes"], c.cpu().numpy().astype(np.int64)[None])
                np.save(rec["mels"], m.to(torch.float32).cpu().numpy().reshape(1, m.shape[-2], m.shape[-1]))
                records.append(rec)
        with open(os.path.join(out_dir, "metadata.jsonl"), "w", encoding="utf-8") as f:
            for rec in records:
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
        return records

    # ------------------------------------------------------------------------------------------------ likelihood of given codes
    def score_codes(self, cond_mel, text_token_rows: List[torch.Tensor], code_rows: List[torch.Tensor], adapter_ids=None,
                    adapter_mix=None):
        """How likely are these codes under this voice?    A ragged batch -- utterance i is
        text_token_rows[i] and code_rows[i] -- through the packed teacher-forced latent pass in the voice of cond_mel (one prompt,
        or a list with one per row, as in infer_batch) and under the rows' adapters, then both output heads through the
        ScoreEngine.  One record per utterance over its REAL positions: its n codes and the first stop (mel), its L tokens and the
        first stop (text): nll_mel (the mean), ppl_mel = exp(nll_mel), acc1 / acc10 / acc20 (the share of mel positions whose
        target is among the head's top 1 / 10 / 20), nll_text, and the per-token arrays mel_nll, mel_rank, mel_best, mel_lse,
        text_nll, text_rank (numpy).  No token is sampled and no logit is stored."""
        if len(code_rows) != len(text_token_rows):
            raise ValueError(f"score_codes: {len(code_rows)} code rows for {len(text_token_rows)} texts")
        g, eng = self.gpt, self.gpt.engine
        B = len(text_token_rows)
        if adapter_ids is not None:
            adapter_ids = eng._row_adapters([-1 if v is None else int(v) for v in adapter_ids], B)   # (None: the base model)
        if adapter_mix is not None:
            adapter_mix = eng._voices(adapter_ids, adapter_mix, B)[1]
        cond_mel = self._check_prompts(cond_mel, B, {}, "score_codes")
        conds, _ = self._prompt_features(cond_mel, spk=False)
        texts = [t.reshape(-1).cpu().long() for t in text_token_rows]
        codes = [c.reshape(-1).cpu().long() for c in code_rows]
        enc, nc = self._latents(conds, texts, codes, adapter_ids=adapter_ids, adapter_mix=adapter_mix, whole=True)
        # position p of a part predicts its token p; the position behind the last token predicts the first stop
        ri, ci, tgt = ([], []), ([], []), ([], [])
        for i, (t, c) in enumerate(zip(texts, codes)):
            for k, (ids, c0, stop) in enumerate(((t, nc, g.stop_text_token), (c, nc + t.numel() + 2, g.stop_mel_token))):
                ri[k].append(torch.full((ids.numel() + 1,), i))
                ci[k].append(c0 + torch.arange(ids.numel() + 1))
                tgt[k].append(torch.cat([ids, torch.tensor([stop])]))
        se = g.score_engine()
        res = []
        for k, head in enumerate(("text", "mel")):
            rows = enc[torch.cat(ri[k]).to(self.device), torch.cat(ci[k]).to(self.device)]
            res.append({key: v.cpu().numpy() for key, v in se.score(rows, torch.cat(tgt[k]), head=head).items()})
        out, at = [], [0, 0]
        for t, c in zip(texts, codes):
            nt, nm = t.numel() + 1, c.numel() + 1
            tx = {key: v[at[0]: at[0] + nt] for key, v in res[0].items()}
            ml = {key: v[at[1]: at[1] + nm] for key, v in res[1].items()}
            at = [at[0] + nt, at[1] + nm]
            nll = float(ml["nll"].astype(np.float64).mean())
            out.append(dict(nll_mel=nll, ppl_mel=float(np.exp(nll)), acc1=float((ml["rank"] < 1).mean()), acc10=float((ml["rank"] < 10).mean()),
                            acc20=float((ml["rank"] < 20).mean()), nll_text=float(tx["nll"].astype(np.float64).mean()), mel_nll=ml["nll"],
                            mel_rank=ml["rank"], mel_best=ml["best"], mel_lse=ml["lse"], text_nll=tx["nll"], text_rank=tx["rank"]))
        return out

    def text_token_row(self, text):
        """A transcript as the token-id row score_codes takes: a string is tokenized as infer() does; a row is passed on."""
        if isinstance(text, str):
            return torch.tensor(self.tokenizer.convert_tokens_to_ids(self.tokenizer.tokenize(text)), dtype=torch.long)
        return text

    def score_audio(self, cond_mel, texts, audios, srs=None, adapter_ids=None, adapter_mix=None):
        """score_codes of recordings: audio_codes(audios, srs) (the tokenizer: load_tokenizer) against their transcripts `texts`
        (strings, tokenized as infer() does, or token-id rows)."""
        rows = [self.text_token_row(t) for t in texts]
        codes, _ = self.audio_codes(audios, srs)
        return self.score_codes(cond_mel, rows, codes, adapter_ids=adapter_ids, adapter_mix=adapter_mix)

    def rank_voices(self, cond_mel, text, audio_or_codes, voices):
        """Which voice explains these codes best?  One batch with a row per entry of `voices` (adapter ids of the attached bank or
        pool; None or -1: the base model), every row the same text (a string or a token-id row) and the same codes (a code
        tensor, or a recording for audio_codes).  -> [(voice, record of score_codes)] sorted by nll_mel, best first."""
        voices = list(voices)
        if torch.is_tensor(audio_or_codes) and not audio_or_codes.is_floating_point():
            codes = audio_or_codes
        else:
            codes = self.audio_codes([audio_or_codes])[0][0]
        row = self.text_token_row(text)
        recs = self.score_codes(cond_mel, [row] * len(voices), [codes] * len(voices), adapter_ids=voices)
        return sorted(zip(voices, recs), key=lambda vr: vr[1]["nll_mel"])

    # ------------------------------------------------------------------------------------------------ voice fitting
    def fit_voice(self, cond_mel, text_token_rows: List[torch.Tensor], code_rows: List[torch.Tensor], *, rank=4, alpha=8.0, steps=100,
                  batch_rows=4096, lr=5.0e-6, targets=None, text_weight=0.1, dropout=0.2, loraplus_lr_ratio=2.0, weight_decay=0.01,
                  max_grad_norm=1.0, warmup_ratio=0.1, accumulate=1, valid=None, eval_every=10, seed=0, return_report=False,
                  attention="torch"):
        """Train the reference's LoRA (train.py:548-605) on this instance's frozen GPT and return (adapters, scaling) in the
        attach_lora format -- what add_voice, attach_lora_bank, save_voice and score_codes(adapter_ids=...) take (DESIGN.md section
        4.29).  Utterance i is text_token_rows[i] and code_rows[i] (what extract_codes wrote); cond_mel is one prompt or a list with
        one per utterance, conditioned once, without gradient.  The utterances are cut, in order, into padded batches of at most
        batch_rows rows (utterances x the longest); an optimizer step takes `accumulate` of them in turn, `steps` steps in all.
        valid = (text rows, code rows): the score_codes records of the held-out set every eval_every steps and at the end.
        return_report: (adapters, scaling, report) with report["steps"] (loss_text, loss_mel, loss, grad_norm, lr per step) and
        report["valid"].  Every refusal comes before anything is launched.  Nothing of the engine, its bank or its graphs changes -- but
        for valid= without an attached voice pool, which attaches a one-slot pool for each evaluation and detaches it (every attach
        drops the captured graphs): attach a pool first to keep them.  With a prompt per utterance, valid=(texts, codes, prompts).
        attention="hip": the blocks' causal attention, forward and backward, as one ragged HIP launch per block in the place of the
        per-utterance torch loop; the default "torch" is the loop."""
        from indextts.gpt.fit import TARGETS, FitConfig, FitEngine, check_engine, check_rows, plan_batches
        g, eng = self.gpt, self.gpt.engine
        cfg = FitConfig(rank=rank, alpha=float(alpha), targets=tuple(TARGETS if targets is None else targets), dropout=float(dropout),
                        text_weight=float(text_weight), lr=float(lr), loraplus_lr_ratio=float(loraplus_lr_ratio),
                        weight_decay=float(weight_decay), max_grad_norm=max_grad_norm, total_steps=int(steps), warmup_ratio=float(warmup_ratio),
                        seed=int(seed), start_text_token=g.start_text_token, stop_text_token=g.stop_text_token,
                        mel_length_compression=g.mel_length_compression, attention=attention).check()
        check_engine(eng, "fit_voice")
        if int(accumulate) < 1 or int(eval_every) < 1:
            raise ValueError("fit_voice: accumulate and eval_every must be at least 1")
        B = len(text_token_rows)
        rows = check_rows(text_token_rows, code_rows, batch_rows, n_cond=int(g.cond_num), who="fit_voice")   # (the perceiver's latents)
        if valid is not None:
            check_rows(valid[0], valid[1], None, who="fit_voice(valid=)")
            if isinstance(cond_mel, (list, tuple)) and len(valid) < 3:
                raise ValueError("fit_voice(valid=): with a prompt per utterance the held-out set names its own: valid=(texts, codes, prompt "
                                 "or prompts)")
        cond_mel = self._check_prompts(cond_mel, B, {}, "fit_voice")
        with torch.no_grad():
            conds, _ = self._prompt_features(cond_mel, spk=False)
        conds = conds.detach()
        if int(conds.shape[1]) != int(g.cond_num):
            raise RuntimeError(f"fit_voice: the conditioner gave {int(conds.shape[1])} latents, the model is configured for {int(g.cond_num)}")
        fit = FitEngine(eng, g._sd, cfg)
        plan = plan_batches(rows, int(batch_rows))
        batches = [fit.batch(conds if conds.shape[0] == 1 else conds[torch.tensor(ix, device=conds.device)],
                             [text_token_rows[i] for i in ix], [code_rows[i] for i in ix]) for ix in plan]
        report, at = dict(steps=[], valid=[]), 0
        for k in range(int(steps)):
            micro = [batches[(at + j) % len(batches)] for j in range(int(accumulate))]
            at = (at + int(accumulate)) % len(batches)
            report["steps"].append(fit.step(micro))
            if valid is not None and ((k + 1) % int(eval_every) == 0 or k + 1 == int(steps)):
                report["valid"].append(dict(step=k + 1, records=self._score_under(valid[2] if len(valid) > 2 else cond_mel, valid[0], valid[1], fit.voice())))
        adapters, scaling = fit.voice()
        return (adapters, scaling, report) if return_report else (adapters, scaling)

    def _score_under(self, cond_mel, text_rows, code_rows, voice):
        """score_codes of a held-out set under a voice that is in no bank yet: through add_voice / remove_voice when a voice pool is
        attached (nothing else of it changes), else through a one-slot pool attached for the call and detached after it -- which
        drops the engine's captured graphs, as every attach does: the one case in which fit_voice touches the engine."""
        eng = self.gpt.engine
        n = len(text_rows)
        prompt = cond_mel                      # (one prompt, or one per held-out utterance: score_codes checks the list)
        if eng._pool() is not None:
            vid = self.add_voice(*voice)
            try:
                return self.score_codes(prompt, text_rows, code_rows, adapter_ids=[vid] * n)
            finally:
                self.remove_voice(vid)
        if eng.bank is not None:
            raise ValueError("fit_voice(valid=): a fixed adapter bank is attached: attach a voice pool (attach_voice_pool) or detach it")
        rank = max(int(A.shape[0]) for A, _ in voice[0].values())
        self.attach_voice_pool([voice], slots=1, rank=rank)
        try:
            return self.score_codes(prompt, text_rows, code_rows, adapter_ids=[0] * n)
        finally:
            self.detach_voice_pool()

    def fit_voice_from_dir(self, data_dir, cond_mel, **kw):
        """fit_voice on what extract_codes wrote into data_dir: metadata.jsonl (text, codes per clip) and codes/*.npy.  The
        transcripts are tokenized as infer() does.  kw: fit_voice's keywords."""
        meta = os.path.join(data_dir, "metadata.jsonl")
        if not os.path.exists(meta):
            raise ValueError(f"fit_voice_from_dir: {meta} does not exist (extract_codes writes it)")
        texts, codes = [], []
        with open(meta, "r", encoding="utf-8") as f:
            for n, line in enumerate(f):
                if not line.strip():
                    continue
                rec = json.loads(line)
                if "text" not in rec or "codes" not in rec:
                    raise ValueError(f"{meta}:{n + 1}: a record needs text and codes")
                path = rec["codes"] if os.path.isabs(rec["codes"]) or os.path.exists(rec["codes"]) else os.path.join(data_dir, rec["codes"])
                if not os.path.exists(path):
                    path = os.path.join(data_dir, "codes", os.path.basename(rec["codes"]))
                codes.append(torch.from_numpy(np.load(path).astype(np.int64)).reshape(-1))
                texts.append(self.text_token_row(rec["text"]))
        return self.fit_voice(cond_mel, texts, codes, **kw)

    def save_merged(self, path, adapters, scaling):
        """The voice merged into this instance's GPT weights, in the reference's gpt_finetuned.pth format: the checkpoint's own keys
        and dtypes with W + scaling (B A)^T in the place of every adapted weight.  The reference loads it; voice_from_checkpoint of
        it gives the voice back."""
        from indextts.gpt.fit import merged_state_dict
        sd = merged_state_dict(self.gpt._sd, adapters, scaling, self.gpt.engine.L)
        if os.path.dirname(path) != "":
            os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(sd, path)
        return path

    def _finish(self, wavs, output_path, start_time, gpt_gen_time, gpt_forward_time, bigvgan_time, sampling_rate=24000, output=None,
                post=None, speed=None, pitch=None):
        end_time = time.perf_counter()
        wav = torch.cat(wavs, dim=1)
        if speed is not None or pitch is not None:  # on the joined sentences: one chain of lags, no seam at a join; before post
            wav = self._prosody_rows([wav.reshape(-1)], [speed], None if pitch is None else [pitch])[0][None]
        if post is not None:        # on the joined sentences, so that a pause across a join is one pause and the level one level
            wav = self._post_rows([wav], post)[0][None]
        wav_length = wav.shape[-1] / sampling_rate
        print(f">> [stats] total: {end_time - start_time:.2f}s (RTF: {(end_time - start_time) / max(wav_length, 1e-9):.4f})")
        print(f"   - GPT generation: {gpt_gen_time:.2f}s")
        print(f"   - GPT forward: {gpt_forward_time:.2f}s")
        print(f"   - vocoder: {bigvgan_time:.2f}s")
        if output is not None:      # the sentences were joined at 24 kHz above: one encode, no filter transient at a join
            arr = self._encode_rows([wav], output)[0].cpu().numpy()
            if output_path:
                if os.path.dirname(output_path) != "":
                    os.makedirs(os.path.dirname(output_path), exist_ok=True)
                write_wav(output_path, arr, output.sample_rate, output.encoding)
                print(f">> [output] saved to: {output_path}")
                return output_path
            return (output.sample_rate, arr)
        wav = wav.cpu()
        if output_path:
            if os.path.isfile(output_path):
                os.remove(output_path)
            if os.path.dirname(output_path) != "":
                os.makedirs(os.path.dirname(output_path), exist_ok=True)
            write_pcm16(output_path, wav.squeeze(0).to(torch.float32).numpy().astype("int16"), sampling_rate)
            print(f">> [output] saved to: {output_path}")
            return output_path
        return (sampling_rate, wav.type(torch.int16).numpy().T)

    def _vocode(self, latent, spk, lens=None):
        wav, _ = self.bigvgan(latent, speaker_embedding=spk, lens=lens)
        return torch.clamp(32767 * wav.squeeze(1), -32767.0, 32767.0)

    # utterances whose lengths are within this ratio share one (ragged) vocoder batch; the padding rows of the shorter ones
    # cost nothing (tiles past a row's end are not computed) but the batch allocates for the longest
    VOCODER_BUCKET_RATIO = 2.0

    def _vocode_ragged(self, lat, spk):
        """lat: list of [T_i, D] latents; spk [1, 1, 512] (one speaker) or [len(lat), 1, 512] (row i's own speaker, gathered per
        bucket).  Returns the list of waveforms [T_i * hop], each bit-identical to
        vocoding that utterance alone (BigVGAN.forward(lens=...)): utterances are sorted by length and vocoded in
        buckets of similar length -- one launch sequence per bucket instead of one per distinct length."""
        return self._vocode_windows(lat, spk, [(0, int(x.shape[0])) for x in lat])

    def _vocode_windows(self, lat, spk, plans):
        """The samples of the frames [t0_i, t1_i) = plans[i] of utterance i, whose latents so far are lat[i] [T_i, D]; spk as in
        _vocode_ragged.  Utterance i is vocoded over the window [max(0, t0_i - left), min(T_i, t1_i + right)) of
        BigVGAN.receptive_halo(), as BigVGAN.vocode_window does it alone: the windows are sorted by length and run in buckets
        of similar length, zero-padded to the bucket's longest (BigVGAN.forward(lens=...): every element's samples are, bit for
        bit, those of that window vocoded alone), and each is cut to [t0_i, t1_i).  Returns the list of fp32 waveforms
        [(t1_i - t0_i) * hop] in the int16 range.  A window clipped at T_i ends at a true edge only when T_i is the utterance's
        length: the caller plans a frame once the `right` frames behind it exist (stream_plan).  plans (0, T_i) are the whole
        utterances: _vocode_ragged."""
        outs = [None] * len(lat)
        per_row = spk.shape[0] != 1
        if per_row and spk.shape[0] != len(lat):
            raise ValueError(f"{spk.shape[0]} speaker embeddings for {len(lat)} utterances")
        if len(plans) != len(lat) or any(not 0 <= t0 <= t1 <= int(x.shape[0]) for x, (t0, t1) in zip(lat, plans)):
            raise ValueError(f"_vocode_windows: frames {list(plans)} of utterances of {[int(x.shape[0]) for x in lat]}")
        left, right = self.bigvgan.receptive_halo()
        win = [(max(0, t0 - left), min(int(x.shape[0]), t1 + right)) if t1 > t0 else (0, 0) for x, (t0, t1) in zip(lat, plans)]
        spk_all = spk
        order = sorted(range(len(lat)), key=lambda i: win[i][1] - win[i][0])
        k = 0
        while k < len(order):
            t_min = win[order[k]][1] - win[order[k]][0]
            if t_min == 0:
                outs[order[k]] = torch.zeros(0, device=self.device)
                k += 1
                continue
            e = k
            while e < len(order) and win[order[e]][1] - win[order[e]][0] <= self.VOCODER_BUCKET_RATIO * t_min:
                e += 1
            idx = order[k:e]
            lens = [win[i][1] - win[i][0] for i in idx]
            t_max = lens[-1]
            if per_row:
                spk = spk_all[torch.tensor(idx, device=spk_all.device)]
            if lens[0] == t_max:
                wav = self._vocode(torch.stack([lat[i][win[i][0]: win[i][1]] for i in idx], 0), spk)
            else:
                x = torch.zeros(len(idx), t_max, lat[idx[0]].shape[1], dtype=lat[idx[0]].dtype, device=lat[idx[0]].device)
                for j, i in enumerate(idx):
                    x[j, : lens[j]] = lat[i][win[i][0]: win[i][1]]
                wav = self._vocode(x, spk, lens=lens)
            hop = wav.shape[1] // t_max
            for j, i in enumerate(idx):
                outs[i] = wav[j, (plans[i][0] - win[i][0]) * hop: (plans[i][1] - win[i][0]) * hop]
            k = e
        return outs

    # ------------------------------------------------------------------------------------------------ public API
    def infer(self, audio_prompt, text, output_path, verbose=False, max_text_tokens_per_sentence=120, speaker_id=None,
              *, output=None, post=None, speed=None, pitch=None, **generation_kwargs):
        """Sentence-by-sentence synthesis (infer.py:779-917).  output (an OutputFormat; None = 24 kHz PCM16 as ever): the
        sentences are joined at 24 kHz on the device and encoded once; with an output_path the WAV carries the format's tag,
        without one the call returns (rate, array in the encoding).  post (a PostProcess, IndexTTS.post_process; None = the
        samples as ever): silence trimmed, pauses capped and the level set on the joined sentences, before output.  speed (a number
        in [0.5, 2.0]; None and 1.0 = the samples as ever): the speaking rate -- 0.8 a fifth slower, 1.25 a quarter faster, at
        the same pitch (WSOLA on the device, indextts/utils/tempo.py) -- on the joined sentences, before post.  pitch (semitones,
        a number in [-12, 12]; None and 0 = the samples as ever): the voice higher or lower at the duration speed sets -- WSOLA at
        speed / 2^(pitch / 12), then a resampler by 2^(pitch / 12) on the device; the formants move with the pitch; the two
        together must keep speed / 2^(pitch / 12) in [0.5, 2.0] -- where speed is applied."""
        IndexTTS._check_output(output, "infer")
        IndexTTS._check_post(post, "infer")
        speed, pitch = IndexTTS._check_speed(speed, "infer"), IndexTTS._check_pitch(pitch, speed, "infer")
        if speaker_id is not None:
            if not self.speaker_list:
                raise ValueError("multi-speaker mode is not enabled; load speaker_info_path first")
            if speaker_id not in self.speaker_list:
                raise ValueError(f"invalid speaker_id: {speaker_id}")
        start_time = time.perf_counter()
        cond_mel = self._prompt(audio_prompt)
        self._set_gr_progress(0.1, "text processing...")
        sentences = self.tokenizer.split_sentences(self.tokenizer.tokenize(text), max_text_tokens_per_sentence)
        gen, max_mel_tokens = self._gen_kwargs(generation_kwargs)
        conds = self._conds(cond_mel, speaker_id)
        spk = self._spk(cond_mel)
        wavs, gpt_gen_time, gpt_forward_time, bigvgan_time, has_warned = [], 0.0, 0.0, 0.0, False
        for n, sent in enumerate(sentences, 1):
            text_tokens = torch.tensor(self.tokenizer.convert_tokens_to_ids(sent), dtype=torch.int32, device=self.device)[None]
            self._set_gr_progress(0.2 + 0.4 * (n - 1) / len(sentences), f"generating... {n}/{len(sentences)}")
            t0 = time.perf_counter()
            codes = self._generate(conds, text_tokens, gen, max_mel_tokens)
            torch.cuda.synchronize()
            gpt_gen_time += time.perf_counter() - t0
            if not has_warned and (codes[:, -1] != self.stop_mel_token).any():
                warnings.warn(f"generation stopped at max_mel_tokens ({max_mel_tokens}); consider shorter sentences",
                              category=RuntimeWarning)
                has_warned = True
            codes, code_lens = self.remove_long_silence(codes)
            if verbose:
                print(f">> codes {tuple(codes.shape)} lens {code_lens.tolist()}")
            self._set_gr_progress(0.2 + 0.4 * n / len(sentences), f"synthesising... {n}/{len(sentences)}")
            t0 = time.perf_counter()
            latent = self._latents(conds, [text_tokens[0]], [codes[0, : int(code_lens[0])]], reuse_prefix=True)[0][None]
            torch.cuda.synchronize()
            gpt_forward_time += time.perf_counter() - t0
            t0 = time.perf_counter()
            wav = self._vocode(latent, spk)
            torch.cuda.synchronize()
            bigvgan_time += time.perf_counter() - t0
            wavs.append(wav.cpu() if output is None and post is None and speed is None and pitch is None else wav)
        self._set_gr_progress(0.9, "saving audio...")
        return self._finish(wavs, output_path, start_time, gpt_gen_time, gpt_forward_time, bigvgan_time, output=output, post=post,
                            speed=speed, pitch=pitch)

    def infer_fast(self, audio_prompt, text, output_path, verbose=False, max_text_tokens_per_sentence=100,
                   sentences_bucket_max_size=4, *, output=None, post=None, speed=None, pitch=None, **generation_kwargs):
        """Bucketed batch synthesis (infer.py:595-777): sentences of similar length are decoded as one left-padded batch;
        latents are computed in one batched pass and vocoded in time-concatenated pairs (chunk_size 2).  output, post, speed, pitch:
        as in infer."""
        IndexTTS._check_output(output, "infer_fast")
        IndexTTS._check_post(post, "infer_fast")
        speed, pitch = IndexTTS._check_speed(speed, "infer_fast"), IndexTTS._check_pitch(pitch, speed, "infer_fast")
        print(">> [infer] fast mode")
        self._set_gr_progress(0, "initialising...")
        start_time = time.perf_counter()
        cond_mel = self._prompt(audio_prompt)
        sentences = self.tokenizer.split_sentences(self.tokenizer.tokenize(text), max_tokens_per_sentence=max_text_tokens_per_sentence)
        gen, max_mel_tokens = self._gen_kwargs(generation_kwargs)
        conds, spk = self._conds(cond_mel), self._spk(cond_mel)
        self._set_gr_progress(0.1, "text processing...")
        buckets = self.bucket_sentences(sentences, bucket_max_size=sentences_bucket_max_size)
        all_tokens = [[torch.tensor(self.tokenizer.convert_tokens_to_ids(it["sent"]), dtype=torch.int32, device=self.device)[None]
                       for it in b] for b in buckets]
        gpt_gen_time = gpt_forward_time = bigvgan_time = 0.0
        total = sum(len(b) for b in buckets)
        done, all_codes = 0, []
        for toks in all_tokens:
            batch = self.pad_tokens_cat(toks) if len(toks) > 1 else toks[0]
            done += len(toks)
            self._set_gr_progress(0.2 + 0.3 * done / total, f"GPT generating... {done}/{total}")
            t0 = time.perf_counter()
            all_codes.append(self._generate(conds, batch, gen, max_mel_tokens))
            torch.cuda.synchronize()
            gpt_gen_time += time.perf_counter() - t0
        self._set_gr_progress(0.5, "computing latents...")
        idxs, text_rows, code_rows, has_warned = [], [], [], False
        for codes_b, toks, b in zip(all_codes, all_tokens, buckets):
            for i in range(codes_b.shape[0]):
                codes = codes_b[i]
                if not has_warned and codes[-1] != self.stop_mel_token:
                    warnings.warn(f"generation stopped at max_mel_tokens ({max_mel_tokens})", category=RuntimeWarning)
                    has_warned = True
                codes, lens = self.remove_long_silence(codes[None])
                idxs.append(b[i]["idx"])
                text_rows.append(toks[i][0])
                code_rows.append(codes[0, : int(lens[0])])
        t0 = time.perf_counter()
        lat = self._latents(conds, text_rows, code_rows)
        torch.cuda.synchronize()
        gpt_forward_time += time.perf_counter() - t0
        lat = [lat[idxs.index(i)] for i in range(len(lat))]
        self._set_gr_progress(0.7, "vocoding...")
        wavs = []
        for i in range(0, len(lat), 2):
            t0 = time.perf_counter()
            wav = self._vocode(torch.cat(lat[i:i + 2], dim=0)[None], spk)
            torch.cuda.synchronize()
            bigvgan_time += time.perf_counter() - t0
            wavs.append(wav.cpu() if output is None and post is None and speed is None and pitch is None else wav)
        self.torch_empty_cache()
        self._set_gr_progress(0.9, "saving audio...")
        return self._finish(wavs, output_path, start_time, gpt_gen_time, gpt_forward_time, bigvgan_time, output=output, post=post,
                            speed=speed, pitch=pitch)

    def infer_batch(self, cond_mel: torch.Tensor, text_token_rows: List[torch.Tensor], max_mel_tokens=600, force_stop=None,
                    seed=1234, return_codes=False, phase_events: dict | None = None, adapter_ids=None, sampling=None,
                    adapter_mix=None, *, output=None, post=None, speed=None, pitch=None, **generation_kwargs):
        """Utterance-batch data path used by bench.py / the multi-GPU sharder (not in the reference API): one shared
        prompt, N independent texts decoded as ONE left-padded batch, one batched latent pass, and one vocoder call per
        group of equal-length utterances (batching unequal lengths would change the tail of the shorter waveforms).
        Returns a list of fp32 waveforms already scaled to the int16 range, like infer.py:892.
        phase_events, if given, receives torch.cuda.Event marks at the phase boundaries.
        adapter_ids (host ints, one per utterance; needs gpt.attach_lora_bank): the voice -- LoRA adapter of the bank, -1 = base
        model -- each utterance is spoken with, in the token loop and in the latent pass.
        adapter_mix (one mix per utterance, exclusive with adapter_ids): a weighted blend of up to four voices of the bank per
        utterance -- None / -1 (base), an id (that voice at weight 1), {id: weight} ("this voice at 0.6": {3: 0.6}; "70 % A, 30 % B":
        {0: 0.7, 1: 0.3}) or a sequence of (id, weight); weights are any finite numbers (GPTEngine.check_adapter_mix).  The mixes
        are data of the captured decode step: no re-attach, no new graph per assignment.
        sampling (a list of dicts, one per utterance, in the order of text_token_rows): each utterance under its own request's
        settings -- any of do_sample, temperature, top_k, top_p, repetition_penalty, seed; what an entry leaves out comes from
        generation_kwargs and seed (gpt.model.row_sampling_params).  num_beams = 1 only.
        cond_mel may be a LIST of [1, 100, T_i] prompt mels, one per utterance (any lengths): every utterance is cloned from its
        own reference audio, as if synthesised alone with that prompt.  Entries that are the same tensor object are one prompt
        and are conditioned once (_prompt_features_rows); nothing is shared between the rows' prefixes in the prefill.  Works
        together with adapter_ids / adapter_mix and sampling; num_beams = 1 only; a list whose length is not the number of utterances is a
        ValueError.  One tensor is one prompt for all utterances, as before.
        output (an OutputFormat; None = the fp32 waveforms above): the waveforms resampled and encoded on the device, all rows in
        one launch -- a list of uint8 / int16 / float32 device tensors.
        post (a PostProcess, IndexTTS.post_process; None = the waveforms as they are): every utterance trimmed, its pauses capped
        and its level set from its own statistics -- voices recorded at different levels come back at one -- in two launches for
        all rows (indextts/utils/post_wave.py), before output.
        speed (a number in [0.5, 2.0], or a list with one entry per utterance, None entries allowed; None and 1.0 = the waveforms
        as they are): the speaking rate of every utterance at the same pitch -- WSOLA on the device, two launches for all rows
        (indextts/utils/tempo.py) -- before post: pauses and levels are judged on what the listener hears.  The codes, and what
        return_codes returns, are those of the plain call.
        pitch (semitones in [-12, 12], or a list with one entry per utterance, None entries allowed; None and 0 = the waveforms
        as they are): every utterance higher or lower at the duration its speed sets -- WSOLA at speed / 2^(pitch / 12), then a
        resampler by 2^(pitch / 12), one more launch for all rows (TempoEngine.shift) -- where speed is applied.  The formants
        move with the pitch.  A row's speed / 2^(pitch / 12) must lie in [0.5, 2.0]."""
        IndexTTS._check_output(output, "infer_batch")
        IndexTTS._check_post(post, "infer_batch")
        n = len(text_token_rows)
        speed, pitch = IndexTTS._check_speed(speed, "infer_batch", n), IndexTTS._check_pitch(pitch, speed, "infer_batch", n)
        st = self._batch_tokens(cond_mel, text_token_rows, max_mel_tokens, force_stop, seed, phase_events, lazy_spk=True,
                                adapter_ids=adapter_ids, sampling=sampling, adapter_mix=adapter_mix, **generation_kwargs)
        outs = self._batch_waveforms(st, phase_events, reuse_prefix=True)   # serial: the KV cache still holds this batch's prompt
        if speed is not None or pitch is not None:
            outs = self._prosody_rows(outs, speed, pitch)
        if post is not None:
            outs = self._post_rows(outs, post)
        if output is not None:
            outs = self._encode_rows(outs, output)
        return (outs, st["rows"]) if return_codes else outs

    # ------------------------------------------------------------------------------------------------ streaming
    def stream_utterance(self, cond_mel, text_tokens, chunk_tokens=32, max_mel_tokens=600, seed=1234, force_stop=None,
                         adapter_ids=None, adapter_mix=None, latent_cache: bool = False, _trace: dict | None = None,
                         *, output=None, **generation_kwargs):
        """ONE utterance as a generator of PCM chunks (fp32 tensors on the device, int16 range, like infer_batch's waveforms) that
        are produced while the token loop is still running; their concatenation is the utterance.
        Every chunk_tokens tokens the loop pauses (GPTEngine.decode_chunks).  With k codes known and no stop token among them,
        the teacher-forced pass runs over them (_latents with reuse_prefix: only the mel rows, over the prompt K / V the
        prefill left in the decode cache; the whole sequence for an FP8 KV cache).  The pass is causal and row i reads the
        codes < i only, so rows 0 .. k-1 are final.  The vocoder's receptive field is finite (BigVGAN.receptive_halo):
        the samples of frame t read the latent frames [t - left, t + right], so the frames [emitted, k - right) are vocoded
        from a window (_vocode_windows: BigVGAN.vocode_window's forward, clamped and cut) and yielded.  At the stop token, or at
        max_mel_tokens, the rest is flushed against the utterance's true end.  All of it is launched on the loop's stream,
        between two bursts; the passes work on buffers of their own (see decode_chunks).  The stream IS stream_batch's with one
        row (_stream_rows, _emit_boundary), its events unwrapped.
        The latent pass is repeated over all k codes at every boundary: quadratic in the utterance length, at most 600 rows
        per pass.  latent_cache=True runs the INCREMENTAL pass instead (_latents_incremental / GPTEngine.latent_append): the
        stream keeps the pass's own keys and values, the prompt rows go through it once and every mel row once, and a boundary
        costs its new rows only.  The cache holds the prompt + max_mel_tokens + 2 positions (GPTEngine.latent_cache says what
        that takes and what it refuses).  Same codes; fp32 latents are the same bits, 16-bit ones differ by the projections'
        split-K factor.
        Silence: the reference's remove_long_silence is not causal -- it shortens silent runs only when the WHOLE row holds
        more than 30 silent tokens, which is known when the loop ends.  The stream applies only its cut at the stop token.  For
        an utterance with at most 30 silent tokens that is all remove_long_silence does, and the stream equals infer_batch.
        num_beams defaults to 1 here (the whole-utterance calls keep the reference's 3) and a larger value is refused.
        adapter_ids / adapter_mix: one-element lists, the utterance's voice of an attached bank, as infer_batch takes them.
        _trace (private: tests, tools): receives "codes" (the utterance's codes, host int64), "frames" (the [t0, t1) of every chunk) and
        "latent" (per chunk, the rows [t0, t1) its window was vocoded from).
        output (an OutputFormat; None = the fp32 chunks above): the chunks at its rate and in its encoding, produced on the device
        with the resampler's state carried from chunk to chunk -- their concatenation is, bit for bit, the whole utterance
        encoded at once (indextts/utils/pcm_out.py); a chunk holds the samples its boundary has determined.
        The checks run when this is called; the device work starts with the first next()."""
        IndexTTS._check_output(output, "stream_utterance")
        IndexTTS._no_post(generation_kwargs, "stream_utterance")
        IndexTTS._no_speed(generation_kwargs, "stream_utterance")
        gen, chunk_tokens, max_mel_tokens, _ = IndexTTS._stream_batch_args(
            1, chunk_tokens, max_mel_tokens, None, adapter_ids, adapter_mix, None, generation_kwargs, who="stream_utterance")
        if isinstance(cond_mel, (list, tuple)):
            raise ValueError("stream_utterance: one utterance has one prompt mel")
        text = torch.as_tensor(text_tokens).reshape(-1).to("cpu", torch.int32)
        if force_stop is not None:
            force_stop = [int(v) for v in torch.as_tensor(force_stop).reshape(-1).tolist()]
            if len(force_stop) != 1:
                raise ValueError("stream_utterance: force_stop holds one entry")

        def chunks():
            eng, rows = self.gpt.engine, (None if _trace is None else {})
            ids = None if adapter_ids is None else eng._row_adapters(adapter_ids, 1)
            mix = None if adapter_mix is None else eng._voices(None, adapter_mix, 1)[1]
            events = self._stream_rows(cond_mel, [text], chunk_tokens, max_mel_tokens, seed, force_stop, ids, mix, None, rows, gen,
                                       bool(latent_cache), who="stream_utterance", output=output)
            try:
                for _, pcm, _ in events:
                    if _trace is not None:        # the one row's trace, flat
                        _trace.update(codes=rows["codes"][0], frames=rows["frames"][0], latent=rows["latent"][0])
                    if pcm.numel():
                        yield pcm
            finally:
                events.close()
        return chunks()

    @staticmethod
    def stream_plan(k: int, emitted: int, right: int, final: bool):
        """The frames a chunk boundary emits: [emitted, hi).  k: the codes known (final: the utterance's length -- the stop token or
        the token limit has been reached); right: the vocoder's halo towards the future.  Before the end a frame is emitted once
        the `right` frames behind it exist; the end flushes the rest."""
        return emitted, (k if final else max(emitted, k - right))

    @staticmethod
    def stream_queue_plan(rows, emitted, right, max_mel_tokens, stop):
        """One boundary of a stream on the host: THE per-row rule of stream_utterance, stream_batch and stream_queue.  rows: records
        with "utt", "k", "codes" and "stopped" (what GPTEngine.decode_refill_chunks reports; stream_batch_plan makes them of a
        decode_chunks poll); emitted: {utt: the frames it has given out} (an utterance not in it has given none).  Returns
        [(utt, k, t0, t1, final)] in the order of `rows` for the utterances that emit now: k = the position of the row's first stop
        token (the cut of remove_long_silence) or its own token count; final = a stop token is there, the loop says the row has
        stopped, or k has reached max_mel_tokens; (t0, t1) = stream_plan(k, emitted[utt], right, final).  A row with nothing to emit
        that is not final is left out; a final row is always there, with t1 == t0 when nothing is left."""
        out = []
        for row in rows:
            hit = np.flatnonzero(row["codes"].numpy() == stop)       # (host codes: numpy is the cheaper of the two here)
            k = int(hit[0]) if hit.size else int(row["k"])
            final = bool(hit.size) or bool(row["stopped"]) or k >= max_mel_tokens
            t0, t1 = IndexTTS.stream_plan(k, emitted.get(row["utt"], 0), right, final)
            if t1 > t0 or final:
                out.append((row["utt"], k, t0, t1, final))
        return out

    @staticmethod
    def stream_batch_plan(codes, emitted, ended, right, max_mel_tokens, stop):
        """stream_queue_plan for one poll of decode_chunks.  codes: int [B, n]; emitted[b]: the frames row b has given out; ended[b]:
        row b has had its last event and is not planned again.  Every other row is a record with k = n that the loop has not
        stopped (a row ends at its stop token, or at n == max_mel_tokens): [(b, k, t0, t1, final)] in ascending b."""
        n, live = int(codes.shape[1]), [b for b in range(int(codes.shape[0])) if not ended[b]]
        return IndexTTS.stream_queue_plan([dict(utt=b, k=n, codes=codes[b], stopped=False) for b in live],
                                          {b: emitted[b] for b in live}, right, max_mel_tokens, stop)

    def _emit_boundary(self, st: "_StreamState", recs):
        """One boundary of ANY stream (stream_utterance, stream_batch, stream_queue): the events [(handle, pcm, last)] of the
        utterances `recs`, in their order.  A record is stream_queue_plan's ("utt": the key st.emitted knows the utterance by, "k",
        "codes" on the host, "stopped") and carries what the passes need: "handle" (what its events and the trace name it by),
        "text", its prompt's "conds" [1, nc, D] and "spk" [1, 1, 512], "voice", "cache_row" (the decode-cache row its prompt lies
        in: st.latent == "reuse") and "lc_row" (its row of a _LatentRows).  The rows are planned (stream_queue_plan); those that
        emit share ONE latent pass (st.latent) and one ragged vocoder call per bucket of similar window lengths
        (_vocode_windows); one prompt for all of them is passed as that tensor, different ones are concatenated.  A final row
        leaves st.emitted, gives its cache row back (a _LatentRows), is warned about when it ran into max_mel_tokens (st.warn)
        and has an empty pcm when nothing was left to flush.  The sources call it through the class, as stream_queue calls
        _check_prompts: of `self` it needs _latents, _latents_incremental, _vocode_windows and device only."""
        plan = IndexTTS.stream_queue_plan(recs, st.emitted, st.right, st.max_mel_tokens, st.stop)
        by = {r["utt"]: r for r in recs}
        emit = [(by[u], k, t0, t1) for u, k, t0, t1, _ in plan if t1 > t0]
        wavs = {}
        if emit:
            rs = [r for r, _, _, _ in emit]
            same = all(r["conds"] is rs[0]["conds"] for r in rs)
            conds = rs[0]["conds"] if same else torch.cat([r["conds"] for r in rs], 0)
            largs = (conds, [r["text"] for r in rs], [r["codes"][:k] for r, k, _, _ in emit])
            voiced = {} if st.voice_kind is None else {st.voice_kind: [r["voice"] for r in rs]}
            if isinstance(st.latent, _LatentRows):
                lats = self._latents_incremental(st.latent, [r["lc_row"] for r in rs], *largs, **voiced)
            elif st.latent == "reuse":
                lats = self._latents(*largs, reuse_prefix=True, cache_rows=[r["cache_row"] for r in rs], **voiced)
            else:
                lats = self._latents(*largs, reuse_prefix=False, **voiced)
            spans = [(t0, t1) for _, _, t0, t1 in emit]
            spk = rs[0]["spk"] if same else torch.cat([r["spk"] for r in rs], 0)
            wavs = dict(zip([r["utt"] for r in rs], self._vocode_windows(lats, spk, spans)))
            if st.trace is not None:
                for r, lat, (t0, t1) in zip(rs, lats, spans):
                    lo, h = max(0, t0 - st.left), r["handle"]
                    st.trace["frames"][h].append((t0, t1))
                    st.trace["latent"][h].append(lat[t0:t1].clone())
                    st.trace["window"][h].append((lo, lat[lo: min(int(lat.shape[0]), t1 + st.right)].clone()))
        events = []
        for u, k, t0, t1, final in plan:
            r = by[u]
            st.emitted[u] = t1
            if final:
                del st.emitted[u]                         # (a stream_queue runs for as long as requests come)
                if isinstance(st.latent, _LatentRows):
                    st.latent.reset(r["lc_row"])          # the row goes to the next utterance
                if st.warn is not None and not bool((r["codes"] == st.stop).any()):
                    warnings.warn(st.warn.format(r["handle"]), category=RuntimeWarning)
                if st.trace is not None:
                    st.trace["codes"][r["handle"]] = r["codes"][:k].clone()
            events.append((r["handle"], wavs[u] if t1 > t0 else torch.zeros(0, device=self.device), final))
        if st.out is not None and events:     # the boundary's rows through ONE launch; a `last` row flushes its carried tail
            enc = st.out.encode([(u, pcm, last) for (u, _, _, _, _), (_, pcm, last) in zip(plan, events)])
            events = [(h, e, last) for (h, _, last), e in zip(events, enc)]
        return events

    # ------------------------------------------------------------------------------------------------ batched streaming
    @staticmethod
    def _stream_batch_args(n_rows, chunk_tokens, max_mel_tokens, force_stop, adapter_ids, adapter_mix, sampling, generation_kwargs,
                           who="stream_batch"):
        """The checks of stream_utterance (n_rows = 1), stream_batch and stream_queue (`who`) that need neither a model nor a
        device: (gen, chunk_tokens, max_mel_tokens, force_stop as n_rows host ints | None)."""
        kw = dict(generation_kwargs)
        kw.setdefault("num_beams", 1)
        gen, _ = IndexTTS._gen_kwargs(kw)
        if kw:
            raise TypeError(f"{who}: unknown generation settings {sorted(kw)}")
        if int(gen["num_beams"]) > 1:
            raise NotImplementedError(f"{who}: beam search picks its hypothesis when the loop ends, so no code is final "
                                      "before that; streaming is built for num_beams = 1")
        if adapter_ids is not None and adapter_mix is not None:
            raise ValueError(f"{who}: adapter_ids or adapter_mix, one of them")
        for name, v in (("adapter_ids", adapter_ids), ("adapter_mix", adapter_mix), ("sampling", sampling)):
            if v is not None and (isinstance(v, (str, dict)) or not hasattr(v, "__len__") or len(v) != n_rows):
                raise ValueError(f"{who}: {name} is a list with one entry per utterance ({n_rows})")
        chunk_tokens, max_mel_tokens = int(chunk_tokens), int(max_mel_tokens)
        if chunk_tokens < 1:
            raise ValueError(f"{who}: chunk_tokens must be at least 1")
        if force_stop is not None:
            force_stop = force_stop.reshape(-1).tolist() if torch.is_tensor(force_stop) else list(force_stop)
            if len(force_stop) != n_rows:
                raise ValueError(f"{who}: force_stop holds one entry per utterance ({n_rows}; None or -1: no forced stop)")
            force_stop = [-1 if v is None else int(v) for v in force_stop]
        return gen, chunk_tokens, max_mel_tokens, force_stop

    def stream_batch(self, cond_mel, text_token_rows, chunk_tokens=32, max_mel_tokens=600, seed=1234, force_stop=None,
                     adapter_ids=None, adapter_mix=None, sampling=None, latent_cache: bool = False, _trace: dict | None = None,
                     *, output=None, **generation_kwargs):
        """stream_utterance for N utterances in ONE token loop: a generator of events (row, pcm, last) -- row: the index into
        text_token_rows; pcm: an fp32 device tensor in the int16 range, the next samples of that utterance; last: this is the
        row's final event (exactly one per row; its pcm is empty when nothing was left to flush).  The concatenation of a row's
        pcm is that utterance, hop * T_row samples; the events of one boundary come in ascending row order.
        One prefill and one decode_chunks(chunk_tokens) over all rows, as infer_batch prefills and decodes them (same graph key as
        decode() at this B: no new capture).  At every boundary (_emit_boundary), each row that has not ended is planned on its own
        (stream_batch_plan: its codes up to its first stop token, its own emitted count, stream_plan unchanged); the rows that emit
        share ONE latent pass (_latents with reuse_prefix over those cache rows; the whole-sequence pass on an FP8 KV cache) and
        one ragged vocoder call per bucket of similar window lengths (_vocode_windows), so a row's chunk is bit for bit
        BigVGAN.vocode_window of the same latents.  Rows end at different tokens; a row that has ended costs nothing further.
        cond_mel (one mel, or a list with one per row), adapter_ids, adapter_mix, sampling: as infer_batch takes and checks them;
        force_stop: one entry per row (None / -1: none).  num_beams defaults to 1 and a larger value is refused, the silence rule is
        the cut at the stop token and the latent pass is repeated per boundary, all as in stream_utterance; the max_mel_tokens
        warning is given once per row that reaches the limit.  latent_cache=True: the incremental latent pass of
        stream_utterance, one cache row per utterance (also over an FP8 KV cache, whose streams otherwise recompute the prompt).
        Closing the generator early abandons the loop; the next prefill() starts from a clean state as after any decode.
        _trace (private: tests, tools) receives, per row, "codes" (host int64), "frames" ([(t0, t1)]), "latent" (per chunk, the rows
        [t0, t1) its window was cut from), "window" (per chunk, (lo, the latent rows [lo, hi) the vocoder ran over)) and "boundaries"
        (the n of every poll the row was planned at).
        output (an OutputFormat): the events' pcm at its rate and in its encoding, as in stream_utterance; the rows of one
        boundary share one launch, and a row's concatenated pcm is infer_batch(output=...)'s for the same codes.
        The checks run when this is called; the device work starts with the first next()."""
        IndexTTS._check_output(output, "stream_batch")
        IndexTTS._no_post(generation_kwargs, "stream_batch")
        IndexTTS._no_speed(generation_kwargs, "stream_batch")
        N = len(text_token_rows)
        gen, chunk_tokens, max_mel_tokens, force_stop = IndexTTS._stream_batch_args(
            N, chunk_tokens, max_mel_tokens, force_stop, adapter_ids, adapter_mix, sampling, generation_kwargs)
        if sampling is not None:
            sampling = row_sampling_params(sampling, N, gen, seed)
        cond_mel = IndexTTS._check_prompts(self, cond_mel, N, gen, "stream_batch")
        texts = [torch.as_tensor(t).reshape(-1).to("cpu", torch.int32) for t in text_token_rows]
        if N == 0:
            return iter(())
        adapter_ids, adapter_mix = self.gpt.engine._voices(adapter_ids, adapter_mix, N)    # (no bank: None, None)
        return self._stream_rows(cond_mel, texts, chunk_tokens, max_mel_tokens, seed, force_stop, adapter_ids, adapter_mix, sampling,
                                 _trace, gen, bool(latent_cache), output=output)

    def _stream_rows(self, cond_mel, texts, chunk_tokens, max_mel_tokens, seed, force_stop, adapter_ids, adapter_mix, sampling, trace, gen,
                     latent_cache=False, who="stream_batch", output=None):
        """stream_batch's generator (and, with one row and who="stream_utterance", stream_utterance's): one prefill, then every poll
        of decode_chunks becomes the records of the rows that have not ended and goes through _emit_boundary."""
        g, eng = self.gpt, self.gpt.engine
        N = len(texts)
        per_row = isinstance(cond_mel, list)      # conds / spk hold a row per utterance: a record carries its own row's
        conds, spk = self._prompt_features(cond_mel)
        batch_h = torch.full((N, max(int(t.numel()) for t in texts)), self.cfg.gpt.stop_text_token, dtype=torch.int32)
        for i, t in enumerate(texts):
            batch_h[i, : t.numel()] = t
        emb, pad = g.prefix_rows(conds, batch_h)
        sp = sampling_params(gen, seed) if sampling is None else sampling
        shared = 0 if per_row or conds.shape[0] != 1 else int(conds.shape[1])    # one prompt: every row starts with the same latents
        eng.prefill(emb, pad, max_mel_tokens, shared_rows=shared, adapter_ids=adapter_ids, adapter_mix=adapter_mix)
        voices = adapter_ids if adapter_mix is None else adapter_mix
        where = "" if who == "stream_utterance" else " in utterance {}"
        st = _StreamState(self.bigvgan.receptive_halo(), g.stop_mel_token, max_mel_tokens,
                          None if voices is None else "adapter_ids" if adapter_mix is None else "adapter_mix", trace,
                          _LatentRows(eng, N, int(emb.shape[1]) + max_mel_tokens + 2) if latent_cache else "reuse",
                          warn=f"generation stopped at max_mel_tokens ({max_mel_tokens}){where}; consider shorter sentences",
                          out=None if output is None else _StreamOut(self._out_engine(), output))
        if trace is not None:
            trace.update(codes=[None] * N, frames=[[] for _ in range(N)], latent=[[] for _ in range(N)],
                         window=[[] for _ in range(N)], boundaries=[[] for _ in range(N)])
        rows = [dict(utt=b, handle=b, stopped=False, text=texts[b], conds=conds[b: b + 1] if per_row else conds,
                     spk=spk[b: b + 1] if per_row else spk, voice=None if voices is None else voices[b], cache_row=b, lc_row=b)
                for b in range(N)]
        live = list(range(N))                     # the rows that have not had their last event
        chunks = eng.decode_chunks(max_mel_tokens, sp, chunk_tokens, force_stop=force_stop)
        try:
            for codes, _ in chunks:
                n, codes = int(codes.shape[1]), codes.unbind(0)
                if trace is not None:
                    for b in live:
                        trace["boundaries"][b].append(n)
                events = IndexTTS._emit_boundary(self, st, [dict(rows[b], k=n, codes=codes[b]) for b in live])
                over = {b for b, _, last in events if last}
                live = [b for b in live if b not in over]
                yield from events
                if not live:
                    return
        finally:
            chunks.close()       # an early close of this generator abandons the loop, as the end of it does

    # ------------------------------------------------------------------------------------------------ streaming queue
    def stream_queue(self, cond_mel, text_token_rows, slots=32, chunk_tokens=32, max_mel_tokens=600, seed=1234, force_stop=None,
                     adapter_ids=None, adapter_mix=None, sampling=None, more=None, latent_cache: bool = False,
                     _trace: dict | None = None, _refused=None, *, output=None, **generation_kwargs):
        """stream_batch over the REFILLED loop of infer_queue: any number of utterances through `slots` decode slots, each
        streamed as PCM while the loop runs, and utterances that arrive after the loop has started enter it.  A generator of
        events (utt, pcm, last) -- the events of stream_batch; utt: the index into text_token_rows, or the handle `more` gave.
        The loop is infer_queue's: the longest texts are prefilled into the slots, then GPTEngine.decode_refill_chunks(
        check_every=chunk_tokens, staged=True) -- same prefill, same feed, same polls and joins, so an utterance's codes are
        infer_queue(slots=slots, check_every=chunk_tokens)'s bit for bit, and no graph is captured that infer_queue would not
        capture.  What could not be placed (the cache budget of a loop) starts a new loop.
        At every poll each row is planned on its OWN token count k (stream_queue_plan: stream_plan per row -- it emits the frames
        [emitted, k - right), and flushes at its first stop token or at max_mel_tokens, with exactly one `last` event).  The rows
        that emit at a poll share one latent pass and one ragged vocoder call per bucket of similar window lengths
        (_vocode_windows), as in stream_batch.  A refilled row's prompt does not lie where latent_mel_rows looks for it, so the
        latent pass is the whole-sequence one (_latents(reuse_prefix=False), as over an FP8 KV cache).  The events of one poll
        come in the order the utterances entered the loop.
        latent_cache=True: the incremental latent pass of stream_utterance, one cache row per decode slot; a slot's row is reset
        when its utterance has had its last event, before the next owner's first rows.  The cache is sized for the longest
        prompt the loop can place (the queue's longest text; with `more`, gpt.max_text_tokens) + max_mel_tokens + 2, and a
        request from more() whose text is longer than that is refused like any other bad request.
        cond_mel (one mel, or a list with one per utterance), adapter_ids / adapter_mix and sampling: taken and checked as
        infer_queue takes and checks them, before anything is launched; force_stop: one entry per utterance (None / -1: none).
        num_beams defaults to 1 and a larger value is refused (stream_utterance says why).  A row that reaches max_mel_tokens is
        stopped there by the loop, as in infer_queue.  Silence: the stream's rule -- the cut at the stop token only (the
        documented divergence from remove_long_silence, see stream_utterance).
        more (a callable, or None = the static queue): called at every boundary (before the first prefill, and after every
        poll).  It returns a list -- usually empty -- of requests that have arrived, or None: no more will come (it is not
        called again).  A request is a dict: "handle" (what the events name it by), "text" (token ids), and optionally "cond_mel"
        (a mel tensor, or an index into this call's cond_mel list; default: this call's one prompt / its first), "voice" (what
        adapter_ids or adapter_mix would hold for it, whichever this call was given), "sampling" (a dict as in `sampling`) and
        "force_stop".  Arrivals wait behind the queue and are fed to the running loop as slots free up.  With `more` the loop
        runs under per-row settings (as with sampling=[{}, ...]) so that an arrival keeps its own, and the pool is sized for the
        longest prompt the model takes (gpt.max_text_tokens) instead of the queue's longest.  An arrival whose prompt is longer
        than the loop can place -- the pool's window, or the positions the loop has passed -- is held back, for a later poll or
        the next loop; nothing is raised mid-loop on its account.  When the queue and the slots are empty and `more` has not
        said None, the generator ENDS (no idle loop spins): the caller calls again when the next request comes.
        The pool is sized with slots_window for that longest prompt + max_mel_tokens + 2 * chunk_tokens, as infer_queue sizes it:
        every admitted row's whole window is dealt at admission (GPTEngine.admit), so the pool cannot be over-committed.
        Closing the generator early abandons the loop (decode_refill_chunks releases the staged rows).
        _trace (private: tests, tools) receives, per utt, "codes" (host int64), "frames" ([(t0, t1)]), "latent" (per chunk, the
        rows [t0, t1)), "window" (per chunk, (lo, the latent rows [lo, hi) the vocoder ran over)), "polls" (the loop's n at every
        poll the utterance was planned at) and "loops" (the number of loops started).
        A request from more() that does not pass its checks raises from the generator (the caller's error, as a bad argument
        is); _refused (private: serve_stream_queue) is a list that receives (handle, error) instead, and the loop goes on.
        output (an OutputFormat): the events' pcm at its rate and in its encoding, as in stream_batch; an utterance keeps its
        resampler state from its first boundary to its last, in whichever slot it runs.
        The checks run when this is called; the device work starts with the first next()."""
        IndexTTS._check_output(output, "stream_queue")
        IndexTTS._no_post(generation_kwargs, "stream_queue")
        IndexTTS._no_speed(generation_kwargs, "stream_queue")
        N = len(text_token_rows)
        gen, chunk_tokens, max_mel_tokens, force_stop = IndexTTS._stream_batch_args(
            N, chunk_tokens, max_mel_tokens, force_stop, adapter_ids, adapter_mix, sampling, generation_kwargs, who="stream_queue")
        if int(slots) < 1:
            raise ValueError("stream_queue: slots must be >= 1")
        if more is not None and not callable(more):
            raise TypeError("stream_queue: more is a callable that returns the requests that have arrived (or None: no more will come)")
        if sampling is not None or more is not None:
            sampling = row_sampling_params([{}] * N if sampling is None else sampling, N, gen, seed)
        cond_mel, reqs, voice_kind = IndexTTS._queue_requests(self, "stream_queue", cond_mel, text_token_rows, gen, force_stop, sampling,
                                                              adapter_ids, adapter_mix)
        if N == 0 and more is None:
            return iter(())
        return self._stream_queue(cond_mel, reqs, int(slots), chunk_tokens, max_mel_tokens, seed, voice_kind, more, _trace, gen, _refused,
                                  bool(latent_cache), output=output)

    def _queue_requests(self, who, cond_mel, text_token_rows, gen, force_stop, sampling, adapter_ids, adapter_mix):
        """What infer_queue and stream_queue (`who`) do with their arguments before anything is launched: the voices are checked
        (named, or no bank is attached), then the prompts (_check_prompts); every utterance becomes a request -- "handle" (its
        index), "text" (host int32), "prompt" (the key of its prompt's features), "stop", "sp" (its checked settings | None) and
        "voice".  Returns (cond_mel as _check_prompts leaves it, the requests in the order given, voice_kind: the keyword that
        names a voice -- the one this call was given -- or None)."""
        N, eng = len(text_token_rows), self.gpt.engine
        voices = voice_kind = None
        if adapter_ids is not None or adapter_mix is not None:
            adapter_ids, adapter_mix = eng._voices(adapter_ids, adapter_mix, N, queue=True)   # (a pool pages a queue's voices)
            voices, voice_kind = (adapter_ids, "adapter_ids") if adapter_mix is None else (adapter_mix, "adapter_mix")
        elif eng.bank is not None:
            raise NotImplementedError(f"{who}: an adapter bank is attached and no voices were named: pass adapter_ids=[...] or "
                                      "adapter_mix=[...], one entry per utterance (adapter_ids=[-1] * N is the base voice)")
        cond_mel = IndexTTS._check_prompts(self, cond_mel, N, gen, who)
        per_row = isinstance(cond_mel, list)
        reqs = [dict(handle=i, text=torch.as_tensor(t).reshape(-1).to("cpu", torch.int32), prompt=i if per_row else 0,
                     stop=-1 if force_stop is None else int(force_stop[i]), sp=None if sampling is None else sampling[i],
                     voice=None if voices is None else voices[i]) for i, t in enumerate(text_token_rows)]
        return cond_mel, reqs, voice_kind

    @staticmethod
    def _longest_first(reqs):
        """The order a queue is served in: the longest texts start, so that every later prompt fits the positions a loop has passed."""
        return sorted(reqs, key=lambda r: -int(r["text"].numel()))

    def _queue_request(self, r, n_seen, cond_mel, feats, seed, gen, voice_kind):
        """A request `more` returned -> the queue's own form, checked on the host; its prompt's features are computed here when
        the call has not seen that mel (eagerly: no graph is captured beside a running loop)."""
        eng = self.gpt.engine
        if not isinstance(r, dict) or "handle" not in r or "text" not in r:
            raise ValueError("stream_queue: a request from more() is a dict with a 'handle' and a 'text'")
        unknown = sorted(set(r) - {"handle", "text", "cond_mel", "voice", "sampling", "force_stop"})
        if unknown:
            raise ValueError(f"stream_queue: a request from more() holds unknown keys {unknown}")
        m = r.get("cond_mel")
        if m is None:
            m = 0
        if torch.is_tensor(m):
            if id(m) not in feats:
                feats[id(m)] = (m, self.gpt.get_conditioning(m, None), self.bigvgan.speaker_embedding(m.transpose(1, 2)))
            prompt = id(m)
        else:
            prompt = int(m)
            if not 0 <= prompt < (len(cond_mel) if isinstance(cond_mel, list) else 0 if cond_mel is None else 1):
                raise ValueError(f"stream_queue: a request from more() names prompt {prompt}, which this call was not given")
        voice = r.get("voice")
        if voice_kind is None:
            if voice is not None:
                raise ValueError("stream_queue: a request from more() names a voice, but this call was given neither adapter_ids nor adapter_mix")
        elif voice_kind == "adapter_ids":
            voice = eng._row_adapters([-1 if voice is None else voice], 1)[0]
        else:
            voice = eng.check_adapter_mix([voice], 1)[0]
        sp = dict(r.get("sampling") or {})
        sp.setdefault("stream", 0 if "seed" in sp else n_seen)      # the call's seed is shared: arrivals must not draw alike
        stop = r.get("force_stop")
        return dict(handle=r["handle"], text=torch.as_tensor(r["text"]).reshape(-1).to("cpu", torch.int32), prompt=prompt,
                    stop=-1 if stop is None else int(stop), sp=row_sampling_params([sp], 1, gen, seed)[0], voice=voice)

    def _refill_loops(self, waiting, feats, slots, ce, max_mel_tokens, sp_scalar, per_row, voice_kind, one_prompt, staged=True,
                      cache_positions=4096, text_cap=0, closed=None, drain=False, idle=None):
        """The refilled loops of infer_queue and stream_queue, ONE set-up for both: a generator of (loop number, entered, record).
        With a voice pool attached a loop starts with as many of the leading requests as name no more distinct voices than the bank
        has slots (GPTEngine.batch_fit) and runs that many decode slots; the others are fed.
        waiting: the queue, a list of requests the caller may append to between two records -- dicts with "text" (host int32),
        "prompt" (key into feats: (mel, conds [1, nc, D], spk)), "stop", "sp" (checked settings | None) and "voice".  The first
        `slots` of it are prefilled, the others fed as slots free up (GPTEngine.decode_refill_chunks; `closed`: its argument);
        what a loop could not place starts the next one.  entered[u] is the request the record's "utt" u names.  drain: every
        loop runs to its end inside GPTEngine.decode_refill and is yielded ONCE, as (loop number, the requests it placed, their
        codes in that order) -- infer_queue's form: a poll then reads only the rows that have stopped.
        one_prompt: every request speaks from ONE prompt, whose rows the prefill shares (a prompt list never does).  text_cap: size
        the pool for prompts with texts of up to that many tokens (an open queue) instead of the first batch's longest; a request longer
        than the loop can place -- the pool's window, the positions the loop has passed -- stays in `waiting` (an open queue only:
        a static one is fed from its head, longest first).  idle(): called
        when a loop has ended with nothing waiting, the caller's last chance to append.  per_row: the loops run under per-row
        settings (every request's "sp"), else under sp_scalar."""
        g, eng = self.gpt, self.gpt.engine
        stop_text = self.cfg.gpt.stop_text_token

        def conds_of(rs):
            if one_prompt:
                return feats[rs[0]["prompt"]][1]
            return torch.cat([feats[r["prompt"]][1] for r in rs], 0)

        def prefixes(rs):
            """(left-padded prefix batch, pad) of the requests `rs` -- one itts_prefix_rows launch"""
            L = max(int(r["text"].numel()) for r in rs)
            bh = torch.full((len(rs), L), stop_text, dtype=torch.int32)
            for j, r in enumerate(rs):
                bh[j, : r["text"].numel()] = r["text"]
            return g.prefix_rows(conds_of(rs), bh)

        def voiced(rs):
            return {} if voice_kind is None else {voice_kind: [r["voice"] for r in rs]}

        number = 0
        while waiting:
            first = waiting[:slots]
            if voice_kind is not None:
                # a voice pool: the prefilled rows speak at once, so only the leading requests whose voices fit the bank's slots
                # together start the loop -- it then runs that many decode slots -- and the others are fed (and wait for a voice)
                first = first[: max(1, eng.batch_fit([r["voice"] for r in first]))]
            del waiting[: len(first)]
            emb, pad = prefixes(first)
            nc = int(feats[first[0]["prompt"]][1].shape[1])
            p_max = max(int(emb.shape[1]), nc + int(text_cap) + 2 if text_cap else 0)     # the longest prompt this loop can place
            shared = nc if one_prompt else 0
            if eng.paged:
                # paged cache: one loop serves the whole queue -- a slot's blocks go back to the pool when its row stops.  The pool
                # holds `slots` windows of (longest prompt + start token + max_mel_tokens + the steps up to the second next poll)
                eng.prefill(emb, pad, max_mel_tokens + ce + 1, shared_rows=shared,
                            slots_window=p_max + 1 + max_mel_tokens + 2 * ce + 2, **voiced(first))
            else:
                # contiguous strips: the loop runs whole blocks of check_every steps, the cache has to hold that many positions
                # past max_mel_tokens; cache positions only grow, so a loop ends when `cache_positions` are used up
                eng.prefill(emb, pad, max(max_mel_tokens + ce + 1, int(cache_positions) - emb.shape[1] - 2),
                            shared_rows=shared, paged=False, **voiced(first))
            number += 1
            entered, cur_n, S = list(first), 1, int(emb.shape[1]) + 1

            def fits(r):
                """the loop can place r at the next join: its window fits the pool's, its prompt the positions the loop has passed"""
                P = nc + int(r["text"].numel()) + 2
                return P <= p_max and P + 1 <= S + cur_n + (ce if staged else 0) - 1

            def feed(k):
                take = [r for r in waiting if closed is None or fits(r)][:k]
                if not take:
                    return []
                for r in take:
                    waiting.remove(r)
                e, p = prefixes(take)
                p = p.tolist()
                entered.extend(take)
                if voice_kind is not None:
                    return [(e[j, p[j]:], r["stop"], r["sp"], r["voice"]) for j, r in enumerate(take)]
                if per_row:
                    return [(e[j, p[j]:], r["stop"], r["sp"]) for j, r in enumerate(take)]
                return [(e[j, p[j]:], r["stop"]) for j, r in enumerate(take)]

            args = (max_mel_tokens, [r["sp"] for r in first] if per_row else sp_scalar, feed)
            kw = dict(force_stop=[r["stop"] for r in first], check_every=ce, staged=bool(staged),
                      positions=None if eng.kv is not None else max(int(cache_positions), eng._S + max_mel_tokens + ce + 1),
                      **({} if voice_kind is None else {"voices": [r["voice"] for r in first]}))
            if drain:
                codes, leftover = eng.decode_refill(*args, **kw)
                back = len(leftover)
                yield number, entered[: len(entered) - back], codes
            else:
                loop = eng.decode_refill_chunks(*args, closed=closed, **kw)
                try:
                    for rec in loop:
                        cur_n = rec["n"]
                        yield number, entered, rec
                finally:
                    loop.close()       # an early close of this generator abandons the loop, as the end of it does
                back = len(eng.refill_leftover)
            if back:               # fed but not placed: back to the head of the queue
                waiting[:0] = entered[len(entered) - back:]
            if not waiting and idle is not None:
                idle()

    def _stream_queue(self, cond_mel, reqs, slots, chunk_tokens, max_mel_tokens, seed, voice_kind, more, trace, gen, refused=None,
                      latent_cache=False, output=None):
        """stream_queue's generator: every poll of the refilled loops (_refill_loops) becomes the records of the slots' utterances,
        keyed (loop number, utt), and goes through _emit_boundary; between two polls the arrivals are taken in."""
        g = self.gpt
        lc_loop = 0                                     # the loop the latent cache (made at the first poll) serves
        lc_text = max([int(getattr(g, "max_text_tokens", 0)) if more is not None else 0] + [int(r["text"].numel()) for r in reqs])
        waiting = IndexTTS._longest_first(reqs)
        n_seen, open_ = len(reqs), more is not None
        per_row = more is not None or any(r["sp"] is not None for r in reqs)
        feats = {}                                      # prompt key -> (mel, conds [1, nc, D], spk [1, 1, 512])
        # a refilled row's prompt does not lie where latent_mel_rows looks for it: the repeated pass is the whole-sequence one
        st = _StreamState(self.bigvgan.receptive_halo(), g.stop_mel_token, max_mel_tokens, voice_kind, trace, "whole",
                          out=None if output is None else _StreamOut(self._out_engine(), output))
        if trace is not None:
            per_utt = lambda: collections.defaultdict(list)   # noqa: E731
            trace.update(codes={}, frames=per_utt(), latent=per_utt(), window=per_utt(), polls=per_utt(), loops=0)

        def arrivals():
            """one call of more(): the new requests go to the back of the queue.  refused (a list; the service form): a request
            that does not pass its checks is put there with its error and disturbs no other; without it the error is the caller's"""
            nonlocal open_, n_seen
            if not open_:
                return
            new = more()
            if new is None:
                open_ = False
                return
            for r in new:
                try:
                    q = self._queue_request(r, n_seen, cond_mel, feats, seed, gen, voice_kind)
                    if latent_cache and int(q["text"].numel()) > lc_text:
                        raise ValueError(f"stream_queue: a request from more() holds {int(q['text'].numel())} text tokens, the latent "
                                         f"cache of this call is sized for {lc_text}")
                    waiting.append(q)
                except Exception as e:  # noqa: BLE001
                    if refused is None:
                        raise
                    refused.append((r.get("handle") if isinstance(r, dict) else None, e))
                n_seen += 1

        arrivals()
        if cond_mel is not None:                        # the call's own prompts: conditioned once, as infer_queue conditions them
            conds, spk = self._prompt_features(cond_mel)
            if isinstance(cond_mel, list):
                for i, m in enumerate(cond_mel):
                    feats[i] = (m, conds[i: i + 1], spk[i: i + 1])
            else:
                feats[0] = (cond_mel, conds, spk)
        one_prompt = more is None and not isinstance(cond_mel, list)       # (an arrival may bring a prompt of its own)
        text_cap = int(getattr(g, "max_text_tokens", 0)) if more is not None else 0   # an open queue: the longest text the model takes
        loops = self._refill_loops(waiting, feats, slots, chunk_tokens, max_mel_tokens, sampling_params(gen, seed), per_row, voice_kind,
                                   one_prompt, text_cap=text_cap, closed=(lambda: not open_) if more is not None else None, idle=arrivals)
        try:
            for number, entered, rec in loops:
                if trace is not None:
                    trace["loops"] = number
                recs = []
                for row in rec["rows"]:
                    r = entered[row["utt"]]
                    _, conds, spk = feats[r["prompt"]]
                    recs.append(dict(utt=(number, row["utt"]), handle=r["handle"], k=row["k"], codes=row["codes"], stopped=row["stopped"],
                                     text=r["text"], conds=conds, spk=spk, voice=r["voice"], cache_row=None, lc_row=row["slot"]))
                    if trace is not None:
                        trace["polls"][r["handle"]].append(rec["n"])
                if latent_cache and recs and lc_loop != number:
                    if lc_loop == 0:
                        st.latent = _LatentRows(g.engine, slots, int(recs[0]["conds"].shape[1]) + lc_text + 2 + max_mel_tokens + 2)
                    else:                               # a new loop has prefilled every slot anew
                        for s in range(slots):
                            st.latent.reset(s)
                    lc_loop = number
                # Every pass a row of this poll needs -- its latent pass or latent-cache append, its vocoder windows, its `last`
                # event -- is launched inside _emit_boundary, BEFORE `loops` is resumed: with a voice pool the refill loop keeps a
                # stopped row's voices pinned until that resumption (GPTEngine.attach_lora_pool) and relies on exactly this order.
                # Work for a stopped row that moves behind the next next(loops) needs a pin of its own.
                yield from IndexTTS._emit_boundary(self, st, recs)
                arrivals()
        finally:
            loops.close()          # an early close of this generator abandons the loop

    def infer_stream(self, audio_prompt, text, max_text_tokens_per_sentence=120, parallel_sentences=1, slots=None,
                     latent_cache: bool = False, *, output=None, **kw):
        """infer() as a generator of (sampling rate, PCM chunk): the text is split into sentences as infer() splits it and the
        sentences are streamed one after another (stream_utterance, whose keywords -- chunk_tokens, seed, the generation
        settings -- pass through).  A chunk is an fp32 device tensor in the int16 range.
        parallel_sentences = P > 1: the sentences go through stream_batch in groups of up to P, one token loop per group, and the
        chunks are still handed out in text order -- what sentence i + 1 produces before sentence i has ended is held back (by
        reference) until then.  One-element force_stop / adapter_ids / adapter_mix stand for every sentence, as they do with P = 1;
        a group is sampled as one batch, so its samples are not those of P = 1.
        slots = S (not None): ALL sentences go through ONE stream_queue(slots=S) -- the refilled loop: a sentence that ends hands
        its slot to the next one instead of idling to the end of its group -- and the chunks are handed out in text order in the
        same way.  parallel_sentences does not apply then.  Without `slots` the call is what it was.
        latent_cache=True: every one of these streams runs the incremental latent pass (stream_utterance says what that is).
        output (an OutputFormat): the chunks at its rate and in its encoding (each sentence is an utterance of its own, as it is
        a stream of its own); the rate yielded is the format's."""
        IndexTTS._check_output(output, "infer_stream")
        IndexTTS._no_post(kw, "infer_stream")
        IndexTTS._no_speed(kw, "infer_stream")
        rate = 24000 if output is None else output.sample_rate
        if output is not None:
            kw = dict(kw, output=output)
        if latent_cache:
            kw = dict(kw, latent_cache=True)
        P = int(parallel_sentences)
        if P < 1:
            raise ValueError("infer_stream: parallel_sentences must be at least 1")
        if slots is not None and int(slots) < 1:
            raise ValueError("infer_stream: slots must be at least 1")
        cond_mel = self._prompt(audio_prompt)
        sentences = self.tokenizer.split_sentences(self.tokenizer.tokenize(text), max_text_tokens_per_sentence)
        rows = [torch.tensor(self.tokenizer.convert_tokens_to_ids(sent), dtype=torch.int32) for sent in sentences]
        if P == 1 and slots is None:
            for ids in rows:
                for pcm in self.stream_utterance(cond_mel, ids, **kw):
                    yield rate, pcm
            return

        def for_each(group):
            """the keywords with the one-element lists repeated for every sentence of `group`"""
            per_row = {k: list(kw[k]) * len(group) for k in ("force_stop", "adapter_ids", "adapter_mix")
                       if kw.get(k) is not None and not isinstance(kw[k], (str, dict)) and hasattr(kw[k], "__len__") and len(kw[k]) == 1}
            return {**kw, **per_row}

        def in_text_order(events, n):
            order = _TextOrder(n)
            for row, pcm, last in events:
                for c in order.push(row, pcm, last):
                    yield rate, c

        if slots is not None:
            if rows:
                yield from in_text_order(self.stream_queue(cond_mel, rows, slots=int(slots), **for_each(rows)), len(rows))
            return
        for s in range(0, len(rows), P):
            group = rows[s: s + P]
            yield from in_text_order(self.stream_batch(cond_mel, group, **for_each(group)), len(group))

    def serve_stream_queue(self, more, slots=32, chunk_tokens=32, max_mel_tokens=600, latent_cache: bool = False, *, output=None):
        """The service form of stream_queue: whole REQUESTS (a prompt file and a text of any number of sentences each) through one
        refilled loop.  more() returns the requests that have arrived (a list, usually empty) or None (no more will come); a
        request is a dict: "handle", "audio_prompt" (a path), "text", and optionally "max_text_tokens_per_sentence", "seed" and
        the per-request settings do_sample / temperature / top_k / top_p / repetition_penalty, and "max_mel_tokens" (at most this
        call's: the request's utterances are stopped there).  A generator of (handle, pcm, last): a request's chunks come in text
        order (what a later sentence produces early is held back, as in infer_stream), `last` with its final one.  A request
        that cannot be taken -- an unreadable prompt, a refused setting -- yields (handle, the exception, True) and disturbs no
        other.  The generator ends when the loop has fallen idle (stream_queue): the caller starts the next one.
        latent_cache: stream_queue's.  output (an OutputFormat): every request's chunks in that format (stream_queue's)."""
        IndexTTS._check_output(output, "serve_stream_queue")
        empty = lambda: torch.zeros(0, device=self.device, dtype=torch.float32 if output is None else output.dtype)   # noqa: E731
        book = {}            # handle -> the text order of its sentences (_TextOrder)
        gen, _ = IndexTTS._gen_kwargs({"num_beams": 1})
        failed = []          # (handle, error | None = nothing to say, True) from here, ((handle, sentence), error) from the queue

        def sentences_of(r):
            """the request's utterances, every one checked as the loop will check it -- what is refused is refused here"""
            IndexTTS._no_speed(r, "serve_stream_queue")      # (a request's own failure, like any refused setting)
            mel = self._prompt(r["audio_prompt"])
            toks = self.tokenizer.split_sentences(self.tokenizer.tokenize(r["text"]), int(r.get("max_text_tokens_per_sentence", 120)))
            own = {k: r[k] for k in ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "seed") if r.get(k) is not None}
            row_sampling_params([own], 1, gen, 1234)
            limit = r.get("max_mel_tokens")
            stop = None if limit is None or int(limit) >= max_mel_tokens else max(int(limit) - 1, 0)
            return [dict(handle=(r["handle"], i), text=torch.as_tensor(self.tokenizer.convert_tokens_to_ids(sent), dtype=torch.int32),
                         cond_mel=mel, sampling=dict(own, stream=i), force_stop=stop) for i, sent in enumerate(toks)]

        def utterances():
            new = more()
            if new is None:
                return None
            out = []
            for r in new:
                try:
                    utts = sentences_of(r)
                    if utts:
                        book[r["handle"]] = _TextOrder(len(utts))
                        out.extend(utts)
                    else:
                        failed.append((r["handle"], None, True))
                except Exception as e:  # noqa: BLE001  (this request's own failure: answered to it alone)
                    failed.append((r["handle"], e, True))
            return out

        def drain_failed():
            while failed:
                item = failed.pop(0)
                h, e = (item[0], item[1]) if len(item) == 3 else (item[0][0], item[1])   # (refused inside the queue: named by its sentence)
                book.pop(h, None)                                # its other sentences, if any run, are dropped
                if h not in done:
                    done.add(h)
                    yield h, (empty() if e is None else e), True

        done = set()         # requests that have had their `last` (a request refused inside the queue may still own rows)
        events = self.stream_queue(None, [], slots=slots, chunk_tokens=chunk_tokens, max_mel_tokens=max_mel_tokens, more=utterances,
                                   _refused=failed, **({"latent_cache": True} if latent_cache else {}),
                                   **({} if output is None else {"output": output}))
        yield from drain_failed()
        for (h, i), pcm, last in events:
            yield from drain_failed()
            order = book.get(h)
            if order is None:                                    # a sentence of a request that has been refused: dropped
                continue
            for c in order.push(i, pcm, last):
                yield h, c, False
            if order.over():
                del book[h]
                done.add(h)
                yield h, empty(), True
        yield from drain_failed()

    def infer_queue(self, cond_mel: torch.Tensor, text_token_rows: List[torch.Tensor], slots=32, max_mel_tokens=600,
                    force_stop=None, seed=1234, return_codes=False, cache_positions=4096, check_every=16, staged=True,
                    phase_events: dict | None = None, sampling=None, adapter_ids=None, adapter_mix=None, *, output=None,
                    post=None, speed=None, pitch=None, **generation_kwargs):
        """Continuous batching (not in the reference API; SURVEY.md section 8e's mitigation for mixed output lengths): any
        number of utterances of one prompt through `slots` decode slots.  The longest texts start; whenever a row emits its
        stop token its codes are taken and its slot is refilled with the next utterance (GPTEngine.decode_refill: the new
        prompt is prefilled into that slot's KV rows right in front of the loop's current cache position, the row gets its
        own clock), so the token loop runs sum(lengths) / slots steps instead of, batch after batch, to each batch's longest
        row.  Then the latent pass and the vocoder run over groups of `slots` finished utterances of similar length.
        num_beams = 1 only.  cache_positions bounds the KV cache (one loop runs at most that many steps past its prompt; the
        queue continues in a fresh loop after that); check_every / staged: how often the loop looks for finished rows and whether
        a refill's prefill runs on a second stream under the loop's next steps (GPTEngine.decode_refill).  Returns the waveforms
        in the order of text_token_rows, as infer_batch.  sampling: as in infer_batch -- an utterance keeps its own settings, seed
        and draw stream in whichever slot, and at whichever step, it enters.  cond_mel: one prompt, or a list with one prompt per
        utterance as in infer_batch -- an utterance takes its own prompt's latents into whichever slot it enters.
        adapter_ids / adapter_mix (one entry per utterance, exclusive, the rules of infer_batch; needs gpt.attach_lora_bank, and with a
        bank attached one of them is needed: adapter_ids=[-1] * N is the base voice): an utterance takes its voice into whichever
        slot, and at whichever step, it enters (GPTEngine.decode_refill(voices=...)), and into its latent pass.
        output (an OutputFormat; None = the fp32 waveforms): as in infer_batch -- all utterances encoded in one launch.
        post (a PostProcess; None = the waveforms as they are): as in infer_batch -- all utterances finished in two launches.
        speed (a number or one entry per utterance; None and 1.0 = as they are): as in infer_batch -- before post.
        pitch (semitones, a number or one entry per utterance; None and 0 = as they are): as in infer_batch -- where speed is."""
        IndexTTS._check_output(output, "infer_queue")
        IndexTTS._check_post(post, "infer_queue")
        n = len(text_token_rows)
        speed, pitch = IndexTTS._check_speed(speed, "infer_queue", n), IndexTTS._check_pitch(pitch, speed, "infer_queue", n)
        gen, _ = self._gen_kwargs(generation_kwargs)
        if int(gen.get("num_beams", 1)) != 1:
            raise NotImplementedError("infer_queue: num_beams = 1 only (beam rows cannot be refilled one at a time)")
        if sampling is not None:        # checked before anything is launched
            sampling = row_sampling_params(sampling, len(text_token_rows), gen, seed)
        cond_mel, reqs, voice_kind = self._queue_requests("infer_queue", cond_mel, text_token_rows, gen, force_stop, sampling,
                                                          adapter_ids, adapter_mix)       # likewise: voices, prompts
        if not text_token_rows:
            return ([], []) if return_codes else []
        if int(slots) < 1:
            raise ValueError("infer_queue: slots must be >= 1")
        self._mark(phase_events, "start")
        conds, spk = self._prompt_features(cond_mel)
        per_row = isinstance(cond_mel, list)      # conds / spk hold a row per utterance: every group below gathers its own
        N = len(reqs)
        texts = [r["text"] for r in reqs]

        def voiced(ids):
            """the keyword that names the voices of the utterances `ids` to _latents() (none without voices)"""
            return {} if voice_kind is None else {voice_kind: [reqs[i]["voice"] for i in ids]}

        feats = {i: (None, conds[i: i + 1], None) for i in range(N)} if per_row else {0: (None, conds, None)}
        waiting = self._longest_first(reqs)
        rows: List[torch.Tensor | None] = [None] * N
        self._mark(phase_events, "conditioned")
        # the loops of stream_queue (_refill_loops), each drained inside GPTEngine.decode_refill
        for _, placed, codes in self._refill_loops(waiting, feats, int(slots), int(check_every), max_mel_tokens, sampling_params(gen, seed),
                                                   sampling is not None, voice_kind, not per_row, staged=staged,
                                                   cache_positions=cache_positions, drain=True):
            for r, c in zip(placed, codes):
                rows[r["handle"]] = c
        self._mark(phase_events, "decoded")
        squeezed = []
        for c in rows:
            cc, ln = self.remove_long_silence(c[None])
            squeezed.append(cc[0, : int(ln[0])].cpu())
        outs: List[torch.Tensor | None] = [None] * N
        order = sorted(range(N), key=lambda i: int(squeezed[i].numel()))
        k = 0
        while k < N:
            ids = order[k: k + slots]
            if voice_kind is not None:      # a voice pool: a group names no more distinct voices than the bank has slots
                ids = ids[: max(1, self.gpt.engine.batch_fit([reqs[i]["voice"] for i in ids]))]
            k += len(ids)
            sel = torch.tensor(ids, device=conds.device) if per_row else None
            lat = self._latents(conds[sel] if per_row else conds, [texts[i] for i in ids], [squeezed[i] for i in ids], **voiced(ids))
            for i, w in zip(ids, self._vocode_ragged(lat, spk[sel] if per_row else spk)):
                outs[i] = w
        self._mark(phase_events, "vocoded")
        if speed is not None or pitch is not None:
            outs = self._prosody_rows(outs, speed, pitch)
        if post is not None:
            outs = self._post_rows(outs, post)
        if output is not None:
            outs = self._encode_rows(outs, output)
        return (outs, squeezed) if return_codes else outs

    @staticmethod
    def _mark(phase_events, name):
        if phase_events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            phase_events[name] = e

    def _batch_tokens(self, cond_mel, text_token_rows, max_mel_tokens=600, force_stop=None, seed=1234, phase_events=None,
                      lazy_spk=False, adapter_ids=None, sampling=None, adapter_mix=None, **generation_kwargs):
        """Stage A of infer_batch: prompt conditioning -> prefill -> sampling loop -> silence squeeze (host).  Everything
        here is latency-bound small launches; it ends with the codes on the host, as infer.py:848-861 does."""
        gen, _ = self._gen_kwargs(generation_kwargs)
        if adapter_ids is not None:     # checked before anything is launched
            adapter_ids = self.gpt.engine._row_adapters(adapter_ids, len(text_token_rows))
            if int(gen.get("num_beams", 1)) > 1:
                raise NotImplementedError("beam search with an adapter bank is not built (num_beams = 1)")
        if adapter_mix is not None:     # likewise
            adapter_mix = self.gpt.engine._voices(adapter_ids, adapter_mix, len(text_token_rows))[1]
            if int(gen.get("num_beams", 1)) > 1:
                raise NotImplementedError("beam search with adapter mixes is not built (num_beams = 1)")
        if sampling is not None:        # checked before anything is launched
            if int(gen.get("num_beams", 1)) > 1:
                raise NotImplementedError("beam search with per-row sampling settings is not built (num_beams = 1)")
            sampling = row_sampling_params(sampling, len(text_token_rows), gen, seed)
        cond_mel = self._check_prompts(cond_mel, len(text_token_rows), gen, "infer_batch")
        self._mark(phase_events, "start")
        conds, spk = self._prompt_features(cond_mel, spk=not lazy_spk)   # lazy_spk: stage B asks for the speaker embedding
        L = max(int(t.numel()) for t in text_token_rows)
        stop = self.cfg.gpt.stop_text_token
        batch_h = torch.full((len(text_token_rows), L), stop, dtype=torch.int32)
        if text_token_rows and text_token_rows[0].is_cuda:
            text_token_rows = [t.cpu() for t in text_token_rows]
        for i, t in enumerate(text_token_rows):
            batch_h[i, : t.numel()] = t.reshape(-1).to(torch.int32)
        g = self.gpt
        emb, pad = g.prefix_rows(conds, batch_h)   # one upload for the whole batch; the padding stays a host tensor
        sp = sampling_params(gen, seed)
        self._mark(phase_events, "conditioned")
        nb = int(gen.get("num_beams", 1))
        shared = int(conds.shape[1]) if conds.shape[0] == 1 else 0   # one prompt: every row starts with the same latents
        if isinstance(cond_mel, list):
            shared = 0                                               # a prompt per row: nothing is shared, kv_share stays cleared
        if nb > 1:
            if force_stop is not None:
                raise NotImplementedError("force_stop is a measurement aid of the num_beams=1 loop")
            sp["length_penalty"] = float(gen.get("length_penalty", 0.0))
            g.engine.prefill_beams(emb, pad, max_mel_tokens, nb, shared_rows=shared)
            self._mark(phase_events, "prefilled")
            codes = g.engine.decode_beam(max_mel_tokens, sp, nb)
        else:
            g.engine.prefill(emb, pad, max_mel_tokens, shared_rows=shared, adapter_ids=adapter_ids, adapter_mix=adapter_mix)
            self._mark(phase_events, "prefilled")
            codes = g.engine.decode(max_mel_tokens, sp if sampling is None else sampling, force_stop=force_stop)
        self._mark(phase_events, "decoded")
        codes_np, lens_h = self._squeeze_silence_host(codes)   # infer.py:848-861 on the host copy: one device-to-host transfer in all
        codes_h = torch.from_numpy(codes_np)
        rows = [codes_h[i, : lens_h[i]] for i in range(codes_h.shape[0])]
        # where the latent pass finds each element's prompt in the KV cache: row b, or row b * num_beams when the beam prefill
        # expanded the rows (beam_kv = "copy")
        crows = [b * nb for b in range(len(rows))] if nb > 1 and g.engine.beam_kv != "table" else None
        return dict(conds=conds, spk=spk, rows=rows, texts=[t.reshape(-1) for t in text_token_rows], cache_rows=crows,
                    cond_mel=cond_mel, adapter_ids=adapter_ids, adapter_mix=adapter_mix)

    def _batch_waveforms(self, st, phase_events=None, reuse_prefix=False):
        """Stage B of infer_batch: batched teacher-forced latent pass + vocoder (large MFMA-bound launches, no host sync).
        With reuse_prefix = False it touches no decode-loop state, so it may run on another stream beside the next batch's
        stage A (BatchPipeline, whose prefill overwrites the KV cache: it must not reuse the prompt's keys / values)."""
        conds, spk = st["conds"], st["spk"]
        if spk is None and isinstance(st["cond_mel"], list):
            spk = self._prompt_features(st["cond_mel"])[1]   # lazy_spk, a prompt per row: one pass per distinct prompt, then kept
        elif spk is None:                                 # lazy_spk: first batch of this prompt
            spk = self._prompt_spk(st["cond_mel"])
            bf = self._batch_feat
            if bf is not None and bf[0] is st["cond_mel"] and bf[2] is conds:
                bf[3] = spk
        lat = self._latents(conds, st["texts"], st["rows"], reuse_prefix=reuse_prefix, cache_rows=st.get("cache_rows"),
                            adapter_ids=st.get("adapter_ids"), adapter_mix=st.get("adapter_mix"))
        self._mark(phase_events, "latents")
        outs = self._vocode_ragged(lat, spk)
        self._mark(phase_events, "vocoded")
        return outs


class BatchTicket:
    """Handle of one batch in flight in a BatchPipeline: result() waits for its vocoder stage and returns the waveforms."""

    def __init__(self, rows, keep):
        self.rows, self._keep = rows, keep
        self._ready = threading.Event()
        self._outs = self._done = self._err = None

    def _set(self, outs, done, err=None):
        self._outs, self._done, self._err = outs, done, err
        self._ready.set()

    def result(self):
        self._ready.wait()
        if self._err is not None:
            raise self._err
        self._done.synchronize()
        self._keep = None
        return self._outs


class BatchPipeline:
    """Two-stage software pipeline over utterance batches (serving schedule; not in the reference API).

    Stage A of a batch (conditioning, prefill, the token loop: ~7 small launches per block per token, latency-bound, the
    matrix cores idle) runs on the caller's thread; its stage B (latent pass + vocoder: large MFMA-bound launches) is
    enqueued by a worker thread on a second HIP stream and overlaps stage A of the NEXT batch.  Results are identical
    to infer_batch(): the two stages share only read-only weights (the latent pass and the vocoder allocate their
    activations per call from the stream-aware allocator, the decode loop owns the KV cache and its state)."""

    def __init__(self, tts: "IndexTTS"):
        self.tts = tts
        lo, hi = 0, -1
        self.stream_a = torch.cuda.Stream(device=tts.device, priority=hi)   # latency-critical token loop
        self.stream_b = torch.cuda.Stream(device=tts.device, priority=lo)   # throughput work
        self._jobs: "queue.Queue" = queue.Queue()
        self._inflight: List[BatchTicket] = []
        self._thread = threading.Thread(target=self._worker, name="itts-stage-b", daemon=True)
        self._thread.start()

    def _worker(self):
        torch.cuda.set_device(self.tts.device)
        while True:
            job = self._jobs.get()
            if job is None:
                return
            st, ticket, a_done = job
            try:
                # graph captures (global error mode) must not see another thread allocating or synchronising
                with nat.CAPTURE_LOCK, torch.no_grad(), torch.cuda.stream(self.stream_b):
                    self.stream_b.wait_event(a_done)
                    outs = self.tts._batch_waveforms(st)
                    done = torch.cuda.Event()
                    done.record()
                ticket._set(outs, done)
            except BaseException as e:  # noqa: BLE001  (surfaced by result())
                ticket._set(None, None, e)

    def submit(self, cond_mel, text_token_rows, **kw) -> BatchTicket:
        """Runs stage A (returns once the codes are on the host) and hands stage B to the worker."""
        self.stream_a.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream_a):
            st = self.tts._batch_tokens(cond_mel, text_token_rows, **kw)
            for t in (st["conds"], st["spk"]):
                t.record_stream(self.stream_b)
            a_done = torch.cuda.Event()
            a_done.record()
        ticket = BatchTicket(st["rows"], st)
        self._inflight = [t for t in self._inflight if not t._ready.is_set()] + [ticket]
        self._jobs.put((st, ticket, a_done))
        return ticket

    def drain(self):
        for t in self._inflight:
            t._ready.wait()
        self._inflight.clear()
        self.stream_a.synchronize()
        self.stream_b.synchronize()

    def close(self):
        self._jobs.put(None)
        self._thread.join()


class RequestPool:
    """Serving concurrency (not in the reference API): several independent utterance batches in flight on one GPU, each on
    its own IndexTTS instance, host thread and HIP stream.  A single request's token loop is a chain of ~170 dependent
    microsecond-scale launches per token and leaves most CUs idle; the loops of different requests interleave on the
    chip (measured on MI355X, batch 32: 1.4x the audio-seconds/s of one request at a time with two in flight).
    Instances come from IndexTTS.replica() (shared read-only weights, private KV cache / state / graphs) or are
    independent objects.  Results are those of infer_batch() on one instance."""

    class _Job:
        def __init__(self):
            self.ready, self.out, self.err = threading.Event(), None, None

        def result(self):
            self.ready.wait()
            if self.err is not None:
                raise self.err
            return self.out

    @classmethod
    def of(cls, tts: "IndexTTS", inflight: int = 2) -> "RequestPool":
        return cls([tts] + [tts.replica() for _ in range(max(1, inflight) - 1)])

    def __init__(self, instances: List["IndexTTS"]):
        """Every instance gets an ordinary HIP stream of its own (streams restricted to disjoint CU subsets were measured in
        round 3 and never beat letting the dispatcher interleave the requests: profiles/r03_pool_cu_masks.txt).  The HIP runtime
        multiplexes a process's streams over GPU_MAX_HW_QUEUES hardware queues (default 4, read when the runtime initialises):
        with more requests in flight than queues two of them share one and run back to back -- export GPU_MAX_HW_QUEUES >=
        len(instances) before the process first touches the GPU (bench.py does for its 4-deep leg: 1 740 instead of 1 400
        audio-s/s)."""
        assert instances, "need at least one instance"
        self.instances = list(instances)
        hwq = int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4)
        if len(self.instances) > hwq:
            warnings.warn(f"RequestPool: {len(self.instances)} requests in flight over GPU_MAX_HW_QUEUES={hwq} hardware queues: "
                          f"some request streams will share a queue (export GPU_MAX_HW_QUEUES={len(self.instances)} before the "
                          f"process initialises the GPU)", RuntimeWarning)
        self._queues = [queue.Queue() for _ in self.instances]
        self._threads = [threading.Thread(target=self._run, args=(i,), name=f"itts-request-{i}", daemon=True)
                         for i in range(len(self.instances))]
        self._next = 0
        for t in self._threads:
            t.start()

    def _run(self, i):
        inst, q = self.instances[i], self._queues[i]
        torch.cuda.set_device(inst.device)
        stream = torch.cuda.Stream(device=inst.device)
        while True:
            item = q.get()
            if item is None:
                return
            job, args, kw = item
            try:
                with torch.no_grad(), torch.cuda.stream(stream):
                    job.out = inst.infer_batch(*args, **kw)
                    stream.synchronize()
            except BaseException as e:  # noqa: BLE001  (surfaced by result())
                job.err = e
            job.ready.set()

    def warm_up(self, *args, rounds=2, **kw):
        """Run `rounds` requests on every instance, ONE INSTANCE AT A TIME: the first calls capture CUDA graphs, and a
        capture (global error mode) must not see another thread allocating or synchronising.  Call it once for every
        (batch size, generation settings, prompt length) combination that will be served concurrently; a capture that
        happens later, while other requests are running, fails that request loudly (result() raises)."""
        for i in range(len(self.instances)):
            for _ in range(rounds):
                self.submit(*args, _instance=i, **kw).result()

    def submit(self, cond_mel, text_token_rows, _instance=None, **kw):
        """Queue one infer_batch(cond_mel, text_token_rows, **kw) on the next instance (round robin); returns a handle
        whose result() blocks until the waveforms are complete."""
        i = self._next % len(self.instances) if _instance is None else _instance
        if _instance is None:
            self._next += 1
        job = RequestPool._Job()
        self._queues[i].put((job, (cond_mel, text_token_rows), kw))
        return job

    def close(self):
        for q in self._queues:
            q.put(None)
        for t in self._threads:
            t.join()
