"""Likelihood scoring without a GPU (libindextts_score.so, indextts/gpt/score.py): the eighth library's ABI
and refusals through ctypes, the plain-torch statement against the fixture the reference wrote (tests/golden/score_small.npz,
made by tests/golden/make_score_golden.py), the alignment rules of UnifiedVoice.score, and the ignore rule."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import torch

import score_refs as SR
import synth
import weights
from test_post_wave_cpu import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ittl_abi_version", "ittl_head_nll", "ittl_last_error", "ittl_target_logit"]


def heads64():
    """mel_head and text_head of the synthetic checkpoint, float64: {name: (W [D, V], b [V])}."""
    sd = dict(weights.gpt_state_dict(2, with_conditioner=False))
    sd.update({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({"text_head.weight": (12001, 1280), "text_head.bias": (12001,)},
                                                                         synth.gpt_param).items()})
    return {n: (sd[f"{n}_head.weight"].double().t().contiguous(), sd[f"{n}_head.bias"].double()) for n in ("mel", "text")}


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_score_library_header_and_table_agree():
    from indextts import _native_score as nl
    hdr = open(os.path.join(ROOT, "include", "indextts_score.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(ittl_[a-z0-9_]+)\s*\(", code))) == sorted(nl.EXPORTED_SYMBOLS) == NAMES
    assert sorted(s for s in dynamic_symbols(nl.LIB_PATH) if s.startswith("itt")) == NAMES
    lib = ctypes.CDLL(nl.LIB_PATH)
    lib.ittl_abi_version.restype = ctypes.c_int
    assert lib.ittl_abi_version() == nl.ABI_VERSION == 1 == int(re.search(r"#define ITTL_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("RANGE", 1024), ("WS_PER_ROW_RANGE", 20), ("F32", 0), ("BF16", 1), ("F16", 2)):
        assert int(re.search(rf"#define ITTL_{name} (\d+)", hdr).group(1)) == value == getattr(nl, name)
    assert (ctypes.sizeof(nl.TargetLogitArgs), ctypes.sizeof(nl.HeadNllArgs)) == (64, 112)
    assert nl.ws_bytes(130, 1024) == 0 and nl.ws_bytes(130, 1025) == 20 * 130 * 2 and nl.pitch(8194) == 8200 and nl.pitch(8) == 8


def test_the_eighth_library_keeps_its_symbols_apart_and_is_built():
    from indextts import (_native, _native_audio as nata, _native_codec as natc, _native_out as nato, _native_post as natp,
                          _native_score as nl, _native_tempo as natm, _native_voice as natv)
    others = (_native, nata, natc, nato, natp, natm, natv)
    lib = ctypes.CDLL(nl.LIB_PATH)
    for other in others:
        assert not any(s.startswith("ittl_") for s in other.EXPORTED_SYMBOLS)
        assert not any(s.startswith("ittl_") for s in dynamic_symbols(other.LIB_PATH))
        for s in other.EXPORTED_SYMBOLS:
            assert not hasattr(lib, s), s
    assert len({m.LIB_PATH for m in others + (nl,)}) == 8 and nl.LIB_PATH.endswith("libindextts_score.so")
    mk = open(os.path.join(ROOT, "index-tts-lora_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(LLIB\)", mk, re.M) and re.search(r"^check:.*\$\(LLIB\)", mk, re.M) and "score.hip" in mk
    assert re.search(r"^\trm -rf .*\$\(LLIB\)", mk, re.M)
    assert "_native_score.lib()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_no_default_path_imports_the_scorer():
    code = ("import sys; import indextts.infer, indextts.cli, indextts.gpt.model; "
            "bad = [m for m in sys.modules if m in ('indextts.gpt.score', 'indextts._native_score')]; print(bad); sys.exit(bool(bad))")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "index-tts-lora_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


FAKE = 0x10000000      # aligned addresses that are never read: every case below is refused before any launch
X, W, B, Y, T, NLL, LSE, BEST, RANK, WS = (FAKE + i * 0x4000000 for i in range(10))


def test_refusals_through_ctypes():
    from indextts import _native_score as nl
    lib = nl.lib()

    def target(**kw):
        a = nl.TargetLogitArgs()
        d = dict(x=X, w=W, b=B, y=Y, t=T, n_rows=130, D=40, V=1030, ldw=1032, dtype=nl.F32)
        d.update(kw)
        for k, v in d.items():
            setattr(a, k, v)
        return a

    def head(**kw):
        a = nl.HeadNllArgs()
        d = dict(x=X, w=W, b=B, y=Y, t=T, nll=NLL, lse=LSE, best=BEST, rank=RANK, ws=WS, ws_bytes=20 * 130 * 2, n_rows=130, D=40, V=1030,
                 ldw=1032, dtype=nl.F32)
        d.update(kw)
        for k, v in d.items():
            setattr(a, k, v)
        return a

    def refused(what, **kw):
        calls = [(lib.ittl_head_nll, head)]
        if not set(kw) - set(f[0] for f in nl.TargetLogitArgs._fields_):
            calls.append((lib.ittl_target_logit, target))
        for fn, make in calls:
            a = make(**kw)
            assert fn(ctypes.byref(a), None) == 1 and what in lib.ittl_last_error(), (kw, lib.ittl_last_error())

    assert lib.ittl_head_nll(None, None) == 1 and b"null argument struct" in lib.ittl_last_error()
    assert lib.ittl_target_logit(None, None) == 1 and b"null argument struct" in lib.ittl_last_error()
    for name in ("x", "w", "b", "y"):
        refused(b"null pointer", **{name: None})
    for name in ("t", "nll", "lse", "best", "rank"):
        a = head(**{name: None})
        assert lib.ittl_head_nll(ctypes.byref(a), None) == 1 and b"null pointer" in lib.ittl_last_error()
    a = target(t=None)
    assert lib.ittl_target_logit(ctypes.byref(a), None) == 1 and b"4-byte aligned buffer" in lib.ittl_last_error()
    refused(b"16-byte aligned", x=X + 4)
    refused(b"16-byte aligned", w=W + 8)
    refused(b"4-byte aligned", b=B + 2)
    refused(b"4-byte aligned", y=Y + 1)
    refused(b"4-byte aligned", nll=NLL + 2)
    refused(b"4-byte aligned", t=T + 2)
    refused(b"dtype = 3", dtype=3)
    refused(b"dtype = -1", dtype=-1)
    refused(b"ldw = 1029", ldw=1029)                                # ldw < V
    refused(b"ldw = 1036", ldw=1036)                                # not a multiple of 8
    refused(b"D = 0", D=0)
    refused(b"D = 42", D=42)                                        # fp32: a multiple of 4
    refused(b"D = 44", D=44, dtype=nl.BF16)                         # 16-bit: a multiple of 8
    refused(b"D = 4 ", D=4, dtype=nl.F16)
    refused(b"D = 65540", D=65540)
    refused(b"V = 0", V=0)
    refused(b"V = 16777217", V=(1 << 24) + 1, ldw=(1 << 24) + 8)
    refused(b"n_rows must be", n_rows=0)
    refused(b"n_rows must be", n_rows=(1 << 31) - 64)
    refused(b"ws must be", ws=None)                                 # V = 1030 is two ranges
    refused(b"ws must be", ws=WS + 8)
    refused(b"ws too small", ws_bytes=20 * 130 * 2 - 1)
    refused(b"nll overlaps x", nll=X + 4 * (130 * 40 - 1))          # the last element of x
    refused(b"lse overlaps w", lse=W + 4)
    refused(b"best overlaps b", best=B + 4 * 1029)
    refused(b"rank overlaps y", rank=Y)
    refused(b"nll overlaps t", nll=T + 4 * 129)
    refused(b"lse overlaps ws", lse=WS + 64)
    a = head(x=WS + 4096)                                           # (ittl_target_logit has no workspace: it would take this x)
    assert lib.ittl_head_nll(ctypes.byref(a), None) == 1 and b"ws overlaps x" in lib.ittl_last_error()
    a = target(t=X + 16)
    assert lib.ittl_target_logit(ctypes.byref(a), None) == 1 and b"t overlaps x" in lib.ittl_last_error()
    refused(b"nll overlaps w", nll=W + 4 * 40 * 1032 - 4)           # the last element of an fp32 w
    # one range needs no workspace: the wrapper's size rule and the library's agree
    assert nl.ws_bytes(5, 1024) == 0


# ------------------------------------------------------------------------------------------------------- the statement
def test_plain_torch_statement_reproduces_the_reference_fixture():
    """head_scores_torch in float64 on the fixture's operands (the reference's own final-norm rows at EVERY position of all three
    utterances, padded positions included, and the synthetic heads) gives the fixture's rank and best exactly and its nll to 1e-12
    (one float64 GEMM against another: the summation order is the BLAS's); the mean of ITS nll over all positions is the loss the
    reference's forward returned, within 1e-9."""
    from indextts.gpt.score import head_scores_torch
    fx = SR.fixture()
    H = heads64()
    for name in ("text", "mel"):
        Wd, bd = H[name]
        x = torch.from_numpy(fx[f"{name}_lat64"])
        assert x.shape[:2] == fx[f"{name}_targets"].shape and x.shape[0] == 3
        got = head_scores_torch(x.reshape(-1, x.shape[-1]), Wd, bd, torch.from_numpy(fx[f"{name}_targets"]).reshape(-1))
        assert np.array_equal(got["rank"].numpy(), fx[f"{name}_rank"].reshape(-1)) and np.array_equal(got["best"].numpy(), fx[f"{name}_best"].reshape(-1))
        for k in ("nll", "lse", "t"):
            assert np.abs(got[k].numpy() - fx[f"{name}_{k}"].reshape(-1)).max() < 1e-12, (name, k)
        assert abs(got["nll"].mean().item() - float(fx[f"loss_{name}_64"])) < 1e-9
        assert abs(got["nll"].float().mean().item() - float(fx[f"loss_{name}_32"])) < 1e-4


def test_alignment_and_padding_follow_the_reference_rules():
    """text_targets / mel_targets as UnifiedVoice.score builds them (gpt/score.aligned_targets) equal the reference's, which the
    fixture recorded, and a reconstruction from the rules: past its length a row is stop tokens (mel length = ceil(wav / 1024) + 1),
    one stop is appended, and the targets are the inputs shifted left with one more stop."""
    from indextts.gpt.score import aligned_targets
    fx = SR.fixture()
    text, codes = torch.from_numpy(fx["text"]), torch.from_numpy(fx["codes"])
    tl = torch.from_numpy(fx["text_lens"])
    ml = torch.ceil(torch.from_numpy(fx["wav_lengths"]).float() / 1024).long() + 1
    assert ml.tolist() == [10, 6, 3]
    for tok, lens, stop, want in ((text, tl, 1, fx["text_targets"]), (codes, ml, 8193, fx["mel_targets"])):
        got = aligned_targets(tok, lens, stop)
        rules = np.full((tok.shape[0], tok.shape[1] + 2), stop, dtype=np.int64)
        for r in range(tok.shape[0]):
            n = min(int(lens[r]), tok.shape[1])
            rules[r, :n] = tok[r, :n].numpy()
        assert np.array_equal(got.numpy(), want) and np.array_equal(rules, want)
    assert (fx["mel_targets"][1, 6:] == 8193).all() and (fx["mel_targets"][1, :6] == fx["codes"][1, :6]).all()


def test_the_ignore_rule():
    from indextts.gpt.score import head_scores_torch
    g = torch.Generator().manual_seed(5)
    x, Wm, b = torch.randn(6, 16, generator=g).double(), torch.randn(16, 24, generator=g).double(), torch.randn(21, generator=g).double()
    Wm[:, 21:] = float("nan")                                       # pad columns are not looked at
    y = torch.tensor([3, -1, 21, 2 ** 31 - 1, 0, 20])
    out = head_scores_torch(x, Wm, b, y)
    ref = SR.reference(x.float(), Wm.float(), b.float(), y, 21, torch.float32)
    for r in (1, 2, 3):
        assert out["nll"][r] == 0 and out["t"][r] == 0 and out["rank"][r] == -1 and 0 <= out["best"][r] < 21 and torch.isfinite(out["lse"][r])
    logits = x @ Wm[:, :21] + b
    for r in (0, 4, 5):
        yy = int(y[r])
        assert out["rank"][r] == (logits[r] > logits[r, yy]).sum() and abs(out["nll"][r] - (torch.logsumexp(logits[r], 0) - logits[r, yy])) < 1e-12
    assert torch.equal(out["best"], logits.argmax(1)) and torch.equal(ref["rank"] < 0, out["rank"] < 0)
    # a tie: the smaller id is the best, and is ahead of the larger one only
    Wm[:, 7], b[7] = Wm[:, 2], b[2]
    out = head_scores_torch(x[[0, 0]], Wm, b, torch.tensor([2, 7]))
    assert out["rank"][1] == out["rank"][0] + 1


# ------------------------------------------------------------------------------------------------------------ command line
class StubTTS:
    """What score_rows asks of an IndexTTS, on the host: counts the tokenizer passes and records the voices asked for."""

    def __init__(self):
        self.code_calls, self.voices_seen = 0, []

    def audio_codes(self, audios):
        self.code_calls += 1
        return [torch.arange(3 + len(a)) for a in audios], None

    def text_token_row(self, text):
        return torch.tensor([2 + ord(ch) for ch in text])

    def score_codes(self, cond_mel, rows, codes, adapter_ids=None):
        self.voices_seen.append(adapter_ids)
        return [dict(nll_mel=1.5, ppl_mel=float(np.exp(1.5)), acc1=0.0, acc10=0.5, acc20=1.0, nll_text=2.0,
                     mel_nll=np.full(c.numel() + 1, 1.5, np.float32), mel_rank=np.arange(c.numel() + 1, dtype=np.int32),
                     mel_best=np.zeros(c.numel() + 1, np.int32), mel_lse=np.zeros(c.numel() + 1, np.float32),
                     text_nll=np.full(r.numel() + 1, 2.0, np.float32), text_rank=np.zeros(r.numel() + 1, np.int32)) for r, c in zip(rows, codes)]


def test_score_command_reads_lists_writes_records_and_refuses(tmp_path, capsys):
    import json

    import pytest

    from indextts import cli
    lst = tmp_path / "list.txt"
    lst.write_text("a.wav\thello\n\n/abs/bb.wav\tworld !\nccc.wav\t\n", encoding="utf-8")
    items = cli.read_audio_list(str(lst))
    assert items == [(str(tmp_path / "a.wav"), "hello"), ("/abs/bb.wav", "world !"), (str(tmp_path / "ccc.wav"), "")]
    bad = tmp_path / "bad.txt"
    bad.write_text("a.wav hello\n", encoding="utf-8")
    with pytest.raises(ValueError, match="bad.txt:1"):
        cli.read_audio_list(str(bad))
    # three clips in chunks of two under two voices: the codes are taken once per chunk, not once per voice
    tts = StubTTS()
    recs = list(cli.score_rows(tts, None, items, voice_ids=(4, 7), voice_names=("a.voice", "b.voice"), batch_clips=2))
    assert tts.code_calls == 2 and tts.voices_seen == [[4, 4], [7, 7], [4], [7]]
    assert len(recs) == 6 and [r["voice"] for r in recs] == ["a.voice", "a.voice", "b.voice", "b.voice", "a.voice", "b.voice"]
    for r in recs:
        back = json.loads(json.dumps(r, ensure_ascii=False))
        assert set(back) == {"audio", "text", "voice", "nll_mel", "ppl_mel", "acc1", "acc10", "acc20", "nll_text", "mel_nll", "mel_rank", "mel_best",
                             "mel_lse", "text_nll", "text_rank"}
        assert isinstance(back["mel_nll"], list) and len(back["mel_nll"]) == len(back["mel_rank"]) and back["nll_mel"] == 1.5
    base = list(cli.score_rows(StubTTS(), None, items[:1]))
    assert len(base) == 1 and base[0]["voice"] is None
    # refusals before any model is loaded: a missing list / prompt / voice file, a malformed list; main() hands --score over
    prompt = tmp_path / "p.wav"
    prompt.write_bytes(b"")
    cfg = tmp_path / "config.yaml"
    cfg.write_text("{}")
    common = ["-v", str(prompt), "--out", str(tmp_path / "o.jsonl"), "-c", str(cfg)]
    for argv, what in ((["--score", str(tmp_path / "none.txt")] + common, "audio list"),
                       (["--score", str(lst), "-v", str(tmp_path / "none.wav"), "--out", "o", "-c", str(cfg)], "prompt"),
                       (["--score", str(lst)] + common + ["--voices", str(tmp_path / "none.voice")], "voice file"),
                       (["--score", str(bad)] + common, "expected `path<TAB>transcript`"),
                       (["--score", str(lst)] + common + ["--batch-clips", "0"], "--batch-clips")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 1 and what in capsys.readouterr().out, argv
    with pytest.raises(SystemExit) as e:                            # -v is required
        cli.main(["--score", str(lst), "--out", "o"])
    assert e.value.code == 2
