"""Voice extraction without a GPU (indextts/gpt/voice_extract.py): the float64 reference of
tests/voice_extract_ref.py recovers the rank of a merged LoRA exactly and lands closer to the trained difference than the
checkpoint itself does (the reference is written on its own; these cases also pin the module's probe width and probe draw to the
reference's, so the two run on the same Omega); the module's refusals and omissions (run over the float64 projector, nothing is launched); the voice
file round trip; and the voice library's ABI -- its header against indextts/_native_voice.py, and the product library, which
exports none of it."""
import ctypes
import os
import re

import pytest
import torch

import voice_extract_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(4, 2.0), (16, 0.5), (8, 1.0)]
SHAPED = {(128, 384): "gpt.h.0.attn.c_attn", (512, 128): "gpt.h.0.mlp.c_proj"}


def rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def base():
    return R.small_base()


@pytest.mark.parametrize("save", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rank,scaling", CASES)
@pytest.mark.parametrize("shape", sorted(SHAPED))
def test_reference_recovers_the_rank_and_beats_the_raw_difference(base, shape, rank, scaling, save):
    key = SHAPED[shape]
    tuned, true = R.merged_checkpoint(base, rank, scaling, save)
    raw = tuned[key + ".weight"].double() - base[key + ".weight"].double()
    assert tuple(raw.shape) == shape
    from indextts.gpt import voice_extract
    index = voice_extract.target_keys(1).index(key)
    c = voice_extract.probe_width(16)
    omega = voice_extract.draw_omega(shape[1], c, 0, index)                        # the module's probe is the one the helper draws
    A, B, rep = R.extract_ref(raw, max_rank=16, gap=8.0, index=index)
    assert c == 32 == rep["q"].shape[1] and omega.dtype == torch.float32 and tuple(omega.shape) == (shape[1], c)
    A2, B2, rep2 = R.extract_ref(raw, max_rank=16, gap=8.0, omega=omega)
    assert torch.equal(A, A2) and torch.equal(B, B2) and rep["ratio"] == rep2["ratio"]
    assert rep["r"] == rank and tuple(A.shape) == (rank, shape[0]) and tuple(B.shape) == (shape[1], rank)
    e_extract, e_raw = rel(A.t() @ B.t(), true[key]), rel(raw, true[key])
    print(f"extract | {shape} r={rank} s={scaling} {save} | ratio {rep['ratio']:.1f} | rank-r {e_extract:.3e} | raw {e_raw:.3e}")
    assert e_extract < e_raw


def run(base, tuned, **kw):
    from indextts.gpt import voice_extract
    return voice_extract.extract(base, tuned, 1, R.fp64_project, **kw)


def test_module_agrees_with_the_reference_and_omits_what_did_not_change(base):
    tuned, true = R.merged_checkpoint(base, 8, 1.0, torch.float16)
    same = "gpt.h.0.attn.c_proj"
    tuned[same + ".weight"] = base[same + ".weight"].clone()
    adapters, scaling, report = run(base, {"model": tuned})                        # (the wrapper of a saved checkpoint)
    assert scaling == 1.0 and same not in adapters and same not in report
    assert sorted(adapters) == sorted(k for k in true if k != same) and sorted(report) == sorted(adapters)
    from indextts.gpt.voice_extract import target_keys
    for key, (A, B) in adapters.items():
        K, N = base[key + ".weight"].shape
        assert A.dtype == B.dtype == torch.float32 and tuple(A.shape) == (8, K) and tuple(B.shape) == (N, 8)
        raw = tuned[key + ".weight"].double() - base[key + ".weight"].double()
        Ar, Br, rep = R.extract_ref(raw, index=target_keys(1).index(key))
        assert report[key]["r"] == rep["r"] == 8
        assert abs(report[key]["ratio"] - rep["ratio"]) <= 1e-3 * rep["ratio"]
        assert rel(A.double().t() @ B.double().t(), Ar.t() @ Br.t()) < 1e-5        # products, not factors: fp32 storage of Q, A, B
        assert rel(A.double().t() @ B.double().t(), true[key]) < rel(raw, true[key])


def test_refusals(base):
    tuned, _ = R.merged_checkpoint(base, 8, 1.0, torch.float16)
    other = dict(tuned)
    other["mel_embedding.weight"] = (tuned["mel_embedding.weight"].float() + 0.01).half()
    with pytest.raises(ValueError, match=r"outside the LoRA targets.*mel_embedding\.weight"):
        run(base, other)
    assert len(run(base, other, ignore_other=True)[0]) == 4                        # the override
    full = dict(tuned)
    g = torch.Generator().manual_seed(9)
    key = "gpt.h.0.mlp.c_fc"
    full[key + ".weight"] = (base[key + ".weight"].float() + torch.randn(128, 512, generator=g) * 0.01).half()
    with pytest.raises(ValueError, match=r"gpt\.h\.0\.mlp\.c_fc: the difference from the base is not low-rank \(largest singular-value ratio"):
        run(base, full)
    twenty, _ = R.merged_checkpoint(base, 20, 1.0, torch.float16)
    with pytest.raises(ValueError, match=r"at rank 20; needs >= 8 at a rank <= 16"):
        run(base, twenty, max_rank=16)
    assert all(rep["r"] == 20 for rep in run(base, twenty, max_rank=32)[2].values())
    wrong = dict(tuned)
    wrong[key + ".weight"] = tuned[key + ".weight"][:, :256].contiguous()
    launched = []

    def project(*a):
        launched.append(a)
        return R.fp64_project(*a)
    from indextts.gpt import voice_extract
    with pytest.raises(ValueError, match=r"shape mismatch.*gpt\.h\.0\.mlp\.c_fc\.weight: \(128, 256\) against the base's \(128, 512\)"):
        voice_extract.extract(base, wrong, 1, project)
    with pytest.raises(ValueError, match="outside the LoRA targets"):
        voice_extract.extract(base, other, 1, project)
    assert not launched                                                            # both before any launch
    with pytest.raises(ValueError, match=r"max_rank must lie in \[1, 64\]"):
        run(base, tuned, max_rank=65)


def test_voice_file_round_trip_is_bit_equal(base, tmp_path):
    from indextts.infer import IndexTTS
    tuned, _ = R.merged_checkpoint(base, 4, 2.0, torch.float16)
    adapters, scaling, _ = run(base, tuned)
    path = tmp_path / "voice.pt"
    IndexTTS.save_voice(path, adapters, scaling)
    got, sc = IndexTTS.load_voice(path)
    assert sc == scaling and sorted(got) == sorted(adapters)
    for key, (A, B) in adapters.items():
        assert got[key][0].dtype == A.dtype and torch.equal(got[key][0], A) and torch.equal(got[key][1], B)
    torch.save({"adapters": {}, "scaling": 1.0, "extra": 1}, path)
    with pytest.raises(ValueError, match="not a voice file"):
        IndexTTS.load_voice(path)


def built():
    from indextts import _native, _native_voice
    if not (os.path.exists(_native.LIB_PATH) and os.path.exists(_native_voice.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return _native, _native_voice


def test_voice_library_header_and_table_agree():
    _native, natv = built()
    hdr = open(os.path.join(ROOT, "include", "indextts_voice.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(ittv_[a-z0-9_]+)\s*\(", code)))
    assert syms == sorted(natv.EXPORTED_SYMBOLS) == ["ittv_abi_version", "ittv_delta_project", "ittv_last_error"]
    assert not re.search(r"\bitts_", code, flags=re.I)                             # nothing the product header's symbol scan matches
    lib = ctypes.CDLL(natv.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/indextts_voice.h but not exported"
    lib.ittv_abi_version.restype = ctypes.c_int
    assert lib.ittv_abi_version() == natv.ABI_VERSION == int(re.search(r"#define ITTV_ABI_VERSION (\d+)", hdr).group(1))
    assert ctypes.sizeof(natv.DeltaArgs) == 72                                      # 6 ints, 5 pointers, one int64 (LP64)
    assert natv.DELTA_WS_BYTES == (16 << 20) + (64 << 10) and "((int64_t)(16 << 20) + (64 << 10))" in hdr
    assert (natv.F32, natv.BF16, natv.F16) == tuple(int(re.search(rf"#define ITTV_{n} (\d+)", hdr).group(1)) for n in ("F32", "BF16", "F16"))
    # refused, not launched: a null struct member, and K = 24
    a = natv.DeltaArgs()
    lib.ittv_delta_project.restype, lib.ittv_last_error.restype = ctypes.c_int, ctypes.c_char_p
    lib.ittv_delta_project.argtypes = [ctypes.POINTER(natv.DeltaArgs), ctypes.c_void_p]
    assert lib.ittv_delta_project(ctypes.byref(a), None) == 1 and b"null pointer" in lib.ittv_last_error()
    for f in ("wt", "wb", "x", "y", "ws"):
        setattr(a, f, 4096)
    a.K, a.N, a.c, a.ws_bytes = 24, 16, 16, natv.DELTA_WS_BYTES
    assert lib.ittv_delta_project(ctypes.byref(a), None) == 1 and b"multiples of 16 (got K=24 N=16)" in lib.ittv_last_error()
    with pytest.raises(_native.NativeError, match="device tensors"):
        natv.delta_project(torch.zeros(16, 16), torch.zeros(16, 16), torch.zeros(16, 16), False, torch.zeros(8, dtype=torch.uint8))


def test_product_library_exports_no_voice_symbol():
    _native, natv = built()
    assert b"ittv_" not in open(_native.LIB_PATH, "rb").read()
    assert b"ittv_delta_project" in open(natv.LIB_PATH, "rb").read()
    assert not any(s.startswith("ittv_") for s in _native.EXPORTED_SYMBOLS) and len(_native.EXPORTED_SYMBOLS) == 47
