"""The acoustic tokenizer: a log-mel [100, T] to the mel codes of the decoder, with the encoder half of the DVAE
(libindextts_codec.so, include/indextts_codec.h).

The model, from the state dict of the reference's DiscreteVAE (positional_dims 1, kernel_size 3, num_layers 2, ReLU, no
normalization):
    encoder.0.0   conv1d(channels -> hidden, k3, stride 2, pad 1) + ReLU          T1 = (T + 1) // 2
    encoder.1.0   conv1d(hidden -> 2 hidden, k3, stride 2, pad 1) + ReLU          T2 = (T1 + 1) // 2 codes
    encoder.2..   ResBlock: x + net.4(relu(net.2(relu(net.0(x))))), net.0 / net.2 k3, net.4 k1
    encoder.N     conv1d(2 hidden -> codebook_dim, k1)                            z [T2, codebook_dim]
    codebook.embed [codebook_dim, num_tokens]: the code of a frame is argmin_j |z - e_j|^2

encoder_forward and nearest_code are the readable statement, in plain fp32 torch on any device.  CodecEngine is the same on the
device through the C ABI: one ittc_conv per convolution over the whole ragged batch, then ittc_nearest_code.
"""
from __future__ import annotations

import re
import threading

import torch
import torch.nn.functional as F


def code_count(T: int) -> int:
    """The codes of T mel frames: two stride-2 convolutions with pad 1."""
    T = int(T)
    if T < 0:
        raise ValueError(f"code_count: T = {T} frames")
    return ((T + 1) // 2 + 1) // 2


def layer_plan(state_dict):
    """The convolutions of the encoder in order, from the state dict's keys: a list of dicts with `key` (the weight is
    key + ".weight"), taps, stride, relu_out, and for a ResBlock's last convolution residual = True; `block` marks a ResBlock's
    first.  Refuses a state dict that is not the model above."""
    idx = sorted({int(m.group(1)) for k in state_dict for m in [re.match(r"encoder\.(\d+)\.", k)] if m})
    if not idx or idx != list(range(len(idx))) or "codebook.embed" not in state_dict:
        raise ValueError("dvae: the state dict has no encoder.N.* layers and codebook.embed")
    plan = []
    for i in idx:
        if f"encoder.{i}.0.weight" in state_dict:
            plan.append(dict(key=f"encoder.{i}.0", taps=3, stride=2, relu_out=True))
        elif f"encoder.{i}.net.0.weight" in state_dict:
            plan.append(dict(key=f"encoder.{i}.net.0", taps=3, stride=1, relu_out=True, block=True))
            plan.append(dict(key=f"encoder.{i}.net.2", taps=3, stride=1, relu_out=True))
            plan.append(dict(key=f"encoder.{i}.net.4", taps=1, stride=1, relu_out=False, residual=True))
        elif f"encoder.{i}.weight" in state_dict and i == idx[-1]:
            plan.append(dict(key=f"encoder.{i}", taps=1, stride=1, relu_out=False))
        else:
            raise ValueError(f"dvae: encoder.{i} is neither a strided convolution, a ResBlock nor the final projection")
    if sum(p["stride"] == 2 for p in plan) != 2:
        raise ValueError("dvae: the tokenizer is built for num_layers = 2 (two stride-2 convolutions: 4 frames per code)")
    for p in plan:
        w = state_dict[p["key"] + ".weight"]
        if w.dim() != 3 or w.shape[2] != p["taps"] or state_dict[p["key"] + ".bias"].shape != (w.shape[0],):
            raise ValueError(f"dvae: {p['key']}.weight has the shape {tuple(w.shape)} (a conv1d of {p['taps']} taps)")
    return plan


def encoder_forward(state_dict, mel: torch.Tensor) -> torch.Tensor:
    """z [T2, codebook_dim] of a log-mel [channels, T] (T >= 1): the encoder in fp32 torch ops."""
    x = mel.to(torch.float32).unsqueeze(0)
    skip = None
    for p in layer_plan(state_dict):
        w, b = (state_dict[p["key"] + s].to(x.device, torch.float32) for s in (".weight", ".bias"))
        if p.get("block"):
            skip = x
        x = F.conv1d(x, w, b, stride=p["stride"], padding=(p["taps"] - 1) // 2)
        if p.get("residual"):
            x = x + skip
        if p["relu_out"]:
            x = F.relu(x)
    return x[0].t().contiguous()


def half_norms(embed: torch.Tensor) -> torch.Tensor:
    """h[j] = |e_j|^2 / 2 of a codebook [D, J]: float64, rounded once to fp32."""
    return (embed.to(torch.float64).pow(2).sum(0) * 0.5).to(torch.float32)


def nearest_code(z: torch.Tensor, embed: torch.Tensor) -> torch.Tensor:
    """The code of every row of z [n, D] in embed [D, J] (int64): argmax_j z . e_j - |e_j|^2 / 2, the smallest j among equals."""
    z, embed = z.to(torch.float32), embed.to(z.device, torch.float32)
    s = z @ embed - half_norms(embed).to(z.device)
    best = s.max(dim=1, keepdim=True).values
    J = embed.shape[1]
    return torch.where(s == best, torch.arange(J, device=z.device), J).min(dim=1).values


class CodecEngine:
    """encode(mels): the codes of a ragged list of log-mels, one ittc_conv per convolution for all clips and one
    ittc_nearest_code.  Owns the packed weights, biases, codebook and h on `device` (written once) and nothing else that is
    shared: the activations of a call are that call's own, so one engine may serve several threads."""

    def __init__(self, state_dict, device):
        from indextts import _native_codec as natc
        self.natc = natc
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        natc.lib()
        self.plan = layer_plan(state_dict)
        self.layers = []
        for p in self.plan:
            w = state_dict[p["key"] + ".weight"].to(self.device, torch.float32)
            self.layers.append(dict(p, w=natc.pack_weight(w), b=state_dict[p["key"] + ".bias"].to(self.device, torch.float32).contiguous(),
                                    Cin=int(w.shape[1]), Cout=int(w.shape[0])))
        for a, b in zip(self.layers, self.layers[1:]):
            if a["Cout"] != b["Cin"]:
                raise ValueError(f"dvae: {a['key']} gives {a['Cout']} channels and {b['key']} takes {b['Cin']}")
        self.channels = self.layers[0]["Cin"]
        self.embed = state_dict["codebook.embed"].to(self.device, torch.float32).contiguous()
        self.codebook_dim, self.num_tokens = (int(n) for n in self.embed.shape)
        if self.codebook_dim != self.layers[-1]["Cout"]:
            raise ValueError(f"dvae: codebook.embed is {tuple(self.embed.shape)} and the encoder gives {self.layers[-1]['Cout']} channels")
        self.h = half_norms(self.embed)
        self._lock = threading.Lock()
        self.launches = 0

    def _mel(self, m):
        if not torch.is_tensor(m) or m.dtype != torch.float32 or m.device != self.device or m.dim() != 2 or m.shape[0] != self.channels:
            raise ValueError(f"CodecEngine: a mel is an fp32 tensor [{self.channels}, T] on {self.device}")
        if m.shape[1] < 1:
            raise ValueError("CodecEngine: a clip with T = 0 mel frames has no codes")
        return m

    @torch.no_grad()
    def encode(self, mels, return_z: bool = False):
        """mels: fp32 device tensors [channels, T_i], T_i >= 1.  Returns the list of their codes, int64 device tensors
        [code_count(T_i)], each bit-equal to that clip encoded alone; with return_z also the list of z [code_count(T_i),
        codebook_dim] the codes were chosen from."""
        natc = self.natc
        mels = [self._mel(m) for m in mels]
        if not mels:
            return ([], []) if return_z else []
        lens = [int(m.shape[1]) for m in mels]
        x = torch.cat([m.t() for m in mels]).contiguous()                # channels-last, the clips' rows one after another
        skip, n = None, 0
        for L in self.layers:
            out = [natc.out_rows(t, L["stride"]) for t in lens]
            segs, xo, yo = [], 0, 0
            for t, o in zip(lens, out):
                segs.append((xo, t, yo))
                xo, yo = xo + t, yo + o
            arr, raw = natc.table(segs)
            dev = natc.upload(raw, self.device)
            if L.get("block"):
                skip = x
            y = torch.empty(yo, L["Cout"], dtype=torch.float32, device=self.device)
            flags = (natc.RELU_OUT if L["relu_out"] else 0) | (natc.RESIDUAL if L.get("residual") else 0)
            natc.conv(x, L["w"], L["b"], y, arr, dev.data_ptr(), L["taps"], L["stride"], flags, skip if L.get("residual") else None)
            x, lens, n = y, out, n + 1
        rows = x.shape[0]
        code = torch.empty(rows, dtype=torch.int32, device=self.device)
        nb = natc.ws_bytes(rows, self.num_tokens)
        ws = torch.empty(nb, dtype=torch.uint8, device=self.device) if nb else None
        natc.nearest_code(x, self.embed, self.h, code, None, ws)
        with self._lock:
            self.launches += n + 1
        codes = list(code.long().split(lens))
        return (codes, list(x.split(lens))) if return_z else codes
