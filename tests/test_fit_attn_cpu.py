"""The fit's training attention without a device: the float64 restatement of tests/fit_attn_refs.py against
torch autograd over FitEngine._forward's explicit softmax(q k^T / 8) v and against the attention inside tests/fit_refs.py's model;
the configuration's refusals; the C ABI's three statements (header, loader, library) and the row table's host checks."""
import os
import re
import subprocess

import pytest
import torch

import fit_attn_refs as AR
import fit_refs as FR
import synth
import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "indextts_fit.h")
LIBDIR = os.path.join(ROOT, "index-tts-lora_amd", "indextts", "_lib")


def test_restatement_equals_autograd_over_the_explicit_softmax():
    for lengths, H, std in (((17, 1, 33), 2, 1.0), ((65, 2), 3, 4.0)):
        c = AR.case(lengths, H, std_qk=std, seed=3)
        qkv, dout = AR.clean(c)
        out, lse, dx = AR.attention64(qkv, dout, c["segments"], H)
        o2, dx2 = AR.attention_graph(qkv, dout, c["segments"], H, dtype=torch.float64)
        assert AR.rel(out, o2) <= 1e-12 and AR.rel(dx, dx2) <= 1e-12
        for f, n in c["segments"]:                     # lse against logsumexp of the scores, and a one-row segment's dq = dk = 0
            q, k = qkv[f: f + n, :64].double(), qkv[f: f + n, 64 * H: 64 * H + 64].double()
            s = (q @ k.t() * 0.125).masked_fill(~torch.ones(n, n, dtype=torch.bool).tril(), float("-inf"))
            assert (torch.logsumexp(s, 1) - lse[0, f: f + n]).abs().max() <= 1e-12
            if n == 1:
                assert dx[f, : 2 * 64 * H].abs().max() <= 1e-14 and torch.equal(dx[f, 2 * 64 * H:], dout[f].double())
        covered = torch.zeros(c["M"], dtype=torch.bool)
        for f, n in c["segments"]:
            covered[f: f + n] = True
        assert not out[~covered].any() and not dx[~covered].any() and not lse[:, ~covered].any()


class Tapped(FR.Model):
    """tests/fit_refs.py's model with its first block's c_attn output and c_proj input kept, gradients and all."""

    def linear(self, x, key, factors, scaling, masks):
        if key == "gpt.h.0.attn.c_proj":
            x.retain_grad()
            self.att = x
        y = super().linear(x, key, factors, scaling, masks)
        if key == "gpt.h.0.attn.c_attn":
            y.retain_grad()
            self.qkv = y
        return y


def test_restatement_equals_the_attention_inside_the_reference_model():
    sd = dict(weights.gpt_state_dict(2))
    sd.update({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({"text_head.weight": (12001, 1280), "text_head.bias": (12001,)},
                                                                         synth.gpt_param).items()})
    fx = FR.fixture()
    m = Tapped(sd, 2)
    conds = torch.randn(1, 32, 1280, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.5
    conds.requires_grad_(True)
    n_text = int(fx["text_lens"][0])
    with torch.enable_grad():
        o = m.losses(conds, torch.from_numpy(fx["text"][:1, :n_text]), torch.tensor([n_text]), torch.from_numpy(fx["codes"][:1, :9]),
                     torch.tensor([9 * 1024]))
        (0.1 * o["loss_text"] + 0.9 * o["loss_mel"]).backward()
    qkv, att = m.qkv[0].detach(), m.att[0].detach()
    n = qkv.shape[0]
    out, _, dx = AR.attention64(qkv, m.att.grad[0], [(0, n)], 20)
    print(f"{n} rows: out {AR.rel(out, att):.2e}, dqkv {AR.rel(dx, m.qkv.grad[0]):.2e}")
    assert AR.rel(out, att) <= 1e-12 and AR.rel(dx, m.qkv.grad[0]) <= 1e-12


def test_config_refuses_unknown_attention():
    from indextts.gpt.fit import FitConfig
    assert FitConfig().attention == "torch" and FitConfig().check().attention == "torch"
    assert FitConfig(attention="hip").check().attention == "hip"
    for bad in ("HIP", "", None, "flash"):
        with pytest.raises(ValueError, match="attention must be one of"):
            FitConfig(attention=bad).check()
    import inspect
    from indextts.cli import fit_voice_parser
    from indextts.infer import IndexTTS
    assert inspect.signature(IndexTTS.fit_voice).parameters["attention"].default == "torch"
    p = fit_voice_parser()
    base = ["--fit-voice", "d", "-v", "p.wav", "--out", "v.pt"]
    assert p.parse_args(base).fit_attention == "torch" and p.parse_args(base + ["--fit-attention", "hip"]).fit_attention == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--fit-attention", "triton"])


def dynamic_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_loader_and_library_agree():
    from indextts import _native_fit as nf
    text = open(HEADER).read()
    protos = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(ittf_\w+)\(", text, flags=re.M))
    assert protos == set(nf.EXPORTED_SYMBOLS) and {"ittf_attn_fwd", "ittf_attn_bwd", "ittf_attn_ws_bytes"} <= protos
    lib = os.path.join(LIBDIR, "libindextts_fit.so")
    assert {s for s in dynamic_symbols(lib) if s.startswith("ittf_")} == protos
    assert re.search(r"^#define ITTF_ABI_VERSION 2$", text, flags=re.M) and nf.ABI_VERSION == 2
    import ctypes
    L = ctypes.CDLL(lib)
    assert L.ittf_abi_version() == 2
    for name, value in (("ITTF_ATTN_MAX_SEG", nf.ATTN_MAX_SEG), ("ITTF_ATTN_MAX_HEADS", nf.ATTN_MAX_HEADS), ("ITTF_ATTN_MAX_NSEG", nf.ATTN_MAX_NSEG)):
        assert int(re.search(rf"^#define {name} (\d+)", text, flags=re.M).group(1)) == value
    assert nf.ATTN_MAX_SEG >= 2048
    assert ctypes.sizeof(nf.AttnArgs) == 96
    L.ittf_attn_ws_bytes.restype = ctypes.c_int64
    L.ittf_attn_ws_bytes.argtypes = [ctypes.c_int64, ctypes.c_int]
    assert L.ittf_attn_ws_bytes(1000, 20) == nf.attn_ws_bytes(1000, 20) == 80000 and L.ittf_attn_ws_bytes(0, 20) == 0
    others = [f for f in os.listdir(LIBDIR) if f.endswith(".so") and f != "libindextts_fit.so"]
    assert len(others) >= 9
    for f in others:
        assert not [s for s in dynamic_symbols(os.path.join(LIBDIR, f)) if s.startswith("ittf_")], f


def test_row_table_refusals():
    from indextts import _native_fit as nf
    t = nf.attn_rows([(3, 5), (8, 1), (20, 7)], 30)
    assert t.dtype.name == "int64" and t.tolist() == [[3, 5], [8, 1], [20, 7]]
    assert nf.attn_rows([(0, nf.ATTN_MAX_SEG)], nf.ATTN_MAX_SEG).shape == (1, 2)
    with pytest.raises(ValueError, match="rising order"):
        nf.attn_rows([(10, 2), (3, 2)], 30)
    with pytest.raises(ValueError, match="overlaps segment 0"):
        nf.attn_rows([(3, 5), (7, 2)], 30)
    with pytest.raises(ValueError, match="out of range"):
        nf.attn_rows([(3, 5), (28, 3)], 30)
    with pytest.raises(ValueError, match="out of range"):
        nf.attn_rows([(-1, 5)], 30)
    with pytest.raises(ValueError, match="the longest the kernels take"):
        nf.attn_rows([(0, nf.ATTN_MAX_SEG + 1)], 10000)
    with pytest.raises(ValueError, match="has 0 rows"):
        nf.attn_rows([(0, 0)], 30)
    with pytest.raises(ValueError, match="0 segments"):
        nf.attn_rows([], 30)
