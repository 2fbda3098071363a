"""The acoustic tokenizer without a GPU (libindextts_codec.so, indextts/vqvae/dvae.py): the seventh library's
ABI and refusals through ctypes, the functional form and the float64 restatement of tests/codec_refs.py against the fixture the
reference class wrote (tests/golden/dvae_small.npz), the condition on the fixture that lets the GPU tests require equal codes on
every frame, the checkpoint loader, and extract_codes on a host stand-in for the engine."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import codec_refs as R
from test_post_wave_cpu import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ittc_abi_version", "ittc_conv", "ittc_last_error", "ittc_nearest_code"]
VQ_SMALL = dict(channels=100, num_tokens=64, hidden_dim=32, num_resnet_blocks=3, codebook_dim=32, num_layers=2, positional_dims=1,
                kernel_size=3, smooth_l1_loss=True, use_transposed_convs=False)


def state_dict():
    return {k: torch.from_numpy(v) for k, v in R.fixture()["sd"].items()}


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_codec_library_header_and_table_agree():
    from indextts import _native_codec as natc
    hdr = open(os.path.join(ROOT, "include", "indextts_codec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(ittc_[a-z0-9_]+)\s*\(", code))) == sorted(natc.EXPORTED_SYMBOLS) == NAMES
    assert sorted(s for s in dynamic_symbols(natc.LIB_PATH) if s.startswith("itt")) == NAMES
    lib = ctypes.CDLL(natc.LIB_PATH)
    lib.ittc_abi_version.restype = ctypes.c_int
    assert lib.ittc_abi_version() == natc.ABI_VERSION == 1 == int(re.search(r"#define ITTC_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("KSTEP", 32), ("CODE_RANGE", 1024), ("RELU_IN", 1), ("RELU_OUT", 2), ("RESIDUAL", 4)):
        assert int(re.search(rf"#define ITTC_{name} (\d+)", hdr).group(1)) == value == getattr(natc, name)
    assert (R.RELU_IN, R.RELU_OUT, R.RESIDUAL) == (1, 2, 4)
    assert ctypes.sizeof(natc.Seg) == 32 and (ctypes.sizeof(natc.ConvArgs), ctypes.sizeof(natc.NearestCodeArgs)) == (104, 72)


def test_the_seven_libraries_keep_their_symbols_apart():
    from indextts import (_native, _native_audio as nata, _native_codec as natc, _native_out as nato, _native_post as natp,
                          _native_tempo as natm, _native_voice as natv)
    others = (_native, nata, nato, natp, natm, natv)
    for other in others:
        assert not any(s.startswith("ittc_") for s in other.EXPORTED_SYMBOLS)
        assert not any(s.startswith("ittc_") for s in dynamic_symbols(other.LIB_PATH))
    lib = ctypes.CDLL(natc.LIB_PATH)
    for other in others:
        for s in other.EXPORTED_SYMBOLS:
            assert not hasattr(lib, s), s
    paths = [m.LIB_PATH for m in others + (natc,)]
    assert len(set(paths)) == 7 and natc.LIB_PATH.endswith("libindextts_codec.so")


def test_build_names_the_seventh_library():
    mk = open(os.path.join(ROOT, "index-tts-lora_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(CLIB\)", mk, re.M) and re.search(r"^check:.*\$\(CLIB\)", mk, re.M) and "codec.hip" in mk
    assert re.search(r"^\trm -rf .*\$\(CLIB\)", mk, re.M)
    assert "_native_codec.lib()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_no_default_path_imports_the_tokenizer():
    code = ("import sys; import indextts.infer, indextts.cli; "
            "bad = [m for m in sys.modules if m.startswith('indextts.vqvae') or m == 'indextts._native_codec']; print(bad); sys.exit(bool(bad))")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "index-tts-lora_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


FAKE = 0x10000      # an aligned address that is never read: every case below is refused before any launch


def conv_args(natc, segs=((0, 8, 0),), x=FAKE, w=FAKE + 0x100000, bias=FAKE + 0x200000, resid=None, y=FAKE + 0x300000, x_rows=8, y_rows=4,
              Cin=100, Cout=32, taps=3, stride=2, flags=0, w_elems=None, n_seg=None, segs_dev=FAKE + 0x400000):
    arr = (natc.Seg * len(segs))(*[natc.Seg(a, b, c, 0) for a, b, c in segs])
    a = natc.ConvArgs()
    a.x, a.x_rows, a.w, a.bias, a.resid, a.y, a.y_rows = x, x_rows, w, bias, resid, y, y_rows
    a.w_elems = natc.packed_k(taps, Cin) * Cout if w_elems is None else w_elems
    a.Cin, a.Cout, a.taps, a.stride, a.flags = Cin, Cout, taps, stride, flags
    a.n_seg, a.segs, a.segs_dev = len(segs) if n_seg is None else n_seg, arr, segs_dev
    return a, arr


def test_conv_refusals_through_ctypes():
    from indextts import _native_codec as natc
    lib = natc.lib()

    def refused(what, **kw):
        a = conv_args(natc, **kw)
        assert lib.ittc_conv(ctypes.byref(a[0]), None) == 1 and what in lib.ittc_last_error(), lib.ittc_last_error()

    assert lib.ittc_conv(None, None) == 1 and b"null argument struct" in lib.ittc_last_error()
    for name in ("x", "w", "bias", "y", "segs_dev"):
        refused(b"null pointer", **{name: None})
    refused(b"null pointer", flags=natc.RESIDUAL)                                  # a residual asked for and none given
    refused(b"16-byte aligned", x=FAKE + 4)
    refused(b"16-byte aligned", y=FAKE + 0x300000 + 8)
    refused(b"16-byte aligned", w=FAKE + 0x100000 + 4)
    refused(b"16-byte aligned", flags=natc.RESIDUAL, resid=FAKE + 0x500000 + 4)
    refused(b"8-byte aligned", segs_dev=FAKE + 0x400000 + 4)
    refused(b"unknown flags", flags=8)
    for taps in (0, 2, 4, 5):
        refused(b"taps = %d" % taps, taps=taps)
    for stride in (0, 3):
        refused(b"stride = %d" % stride, stride=stride)
    refused(b"Cin = 102", Cin=102)
    refused(b"Cout = 0", Cout=0)
    refused(b"the pack does not match", w_elems=300 * 32)                          # the unpadded K
    refused(b"the pack does not match", Cin=96, w_elems=320 * 32)                  # another layer's pack
    refused(b"the pack does not match", Cout=64, w_elems=320 * 32)
    refused(b"n_seg must be", n_seg=0)
    refused(b"n_seg must be", n_seg=65536)
    refused(b"x_len = 0 rows", segs=((0, 0, 0),))
    refused(b"lies outside x", x_rows=7)
    refused(b"lies outside x", segs=((1, 8, 0),))
    refused(b"lies outside x", segs=((-1, 8, 0),))
    refused(b"lies outside y", y_rows=3)
    refused(b"lies outside y", segs=((0, 8, 1),))
    refused(b"segment 1 lies outside y", segs=((0, 3, 0), (3, 5, 2)))               # 2 + 3 rows in 4
    refused(b"lies outside y", stride=1)                                           # eight rows at stride 1 are eight outputs
    refused(b"y overlaps x", y=FAKE + 4 * 796)                                     # y starts inside x's last 16 bytes
    refused(b"y overlaps x", x=FAKE + 0x300000 + 4 * 124)                          # x starts inside y
    refused(b"y overlaps resid", flags=natc.RESIDUAL, resid=FAKE + 0x300000 + 64)


def near_args(natc, z=FAKE, embed=FAKE + 0x100000, h=FAKE + 0x200000, code=FAKE + 0x300000, score=None, ws=None, ws_bytes=0, n_rows=5, D=32, J=64):
    a = natc.NearestCodeArgs()
    a.z, a.embed, a.h, a.code, a.score, a.ws, a.ws_bytes, a.n_rows, a.D, a.J = z, embed, h, code, score, ws, ws_bytes, n_rows, D, J
    return a


def test_nearest_code_refusals_through_ctypes():
    from indextts import _native_codec as natc
    lib = natc.lib()

    def refused(what, **kw):
        a = near_args(natc, **kw)
        assert lib.ittc_nearest_code(ctypes.byref(a), None) == 1 and what in lib.ittc_last_error(), lib.ittc_last_error()

    assert lib.ittc_nearest_code(None, None) == 1 and b"null argument struct" in lib.ittc_last_error()
    for name in ("z", "embed", "h", "code"):
        refused(b"null pointer", **{name: None})
    refused(b"16-byte aligned", z=FAKE + 8)
    refused(b"16-byte aligned", h=FAKE + 0x200000 + 4)
    refused(b"4-byte aligned", code=FAKE + 0x300000 + 2)
    refused(b"4-byte aligned", score=FAKE + 0x500000 + 1)
    refused(b"n_rows must be", n_rows=0)
    refused(b"D = 30", D=30)
    refused(b"D = 0", D=0)
    refused(b"J = 66", J=66)
    refused(b"ws must be", J=8192)
    refused(b"ws must be", J=8192, ws=FAKE + 0x600000 + 8, ws_bytes=1 << 20)
    refused(b"ws too small", J=8192, ws=FAKE + 0x600000, ws_bytes=8 * 5 * 8 - 1)
    assert natc.ws_bytes(5, 8192) == 320 and natc.ws_bytes(5, 1024) == 0 and natc.ws_bytes(5, 1028) == 80


# ------------------------------------------------------------------------------------------------ the model's statement
@pytest.mark.parametrize("T", range(1, 10))
def test_code_count(T):
    from indextts.vqvae import code_count
    from indextts import _native_codec as natc
    assert code_count(T) == R.code_count(T) == natc.out_rows(natc.out_rows(T, 2), 2) == ((T + 1) // 2 + 1) // 2 == -(-T // 4)
    x = torch.zeros(1, 1, T)
    assert torch.nn.functional.conv1d(torch.nn.functional.conv1d(x, torch.zeros(1, 1, 3), stride=2, padding=1), torch.zeros(1, 1, 3),
                                      stride=2, padding=1).shape[-1] == code_count(T)


def test_the_functional_form_is_the_reference_class():
    from indextts.vqvae import encoder_forward, nearest_code
    fx, sd = R.fixture(), state_dict()
    assert sorted(R.FRAMES) == [1, 2, 3, 4, 5, 37, 160] and R.code_count(37) == 10
    for T in R.FRAMES:
        z = encoder_forward(sd, torch.from_numpy(fx[T]["mel"]))
        assert z.dtype == torch.float32 and tuple(z.shape) == fx[T]["z32"].shape == (R.code_count(T), 32)
        assert torch.allclose(z, torch.from_numpy(fx[T]["z32"]), rtol=1e-5, atol=1e-6)
        codes = nearest_code(z, sd["codebook.embed"])
        assert codes.dtype == torch.int64 and np.array_equal(codes.numpy(), fx[T]["codes"])
        assert np.array_equal(nearest_code(torch.from_numpy(fx[T]["z32"]), sd["codebook.embed"]).numpy(), fx[T]["codes"])
    e = sd["codebook.embed"].clone()
    e[:, 40] = e[:, 7]
    assert nearest_code(e[:, 40][None], e).tolist() == [7]                         # among equal scores the smallest code
    with pytest.raises(ValueError, match="no encoder"):
        encoder_forward({"codebook.embed": e}, torch.zeros(100, 4))


def test_the_restatement_is_the_reference_class_in_double():
    fx = R.fixture()
    for T in R.FRAMES:
        z = R.encoder64(fx["sd"], fx[T]["mel"])
        assert z.shape == fx[T]["z64"].shape and np.max(np.abs(z - fx[T]["z64"])) < 1e-13
        s, b = R.scores(fx[T]["z64"], fx["sd"]["codebook.embed"])
        assert np.array_equal(R.choose(s), fx[T]["codes"])
        assert R.audit(fx[T]["z32"], fx["sd"]["codebook.embed"], fx[T]["codes"]) == ([], R.code_count(T))
    # the variants of the negative controls do compute something else, and the plain form itself
    sd = fx["sd"]
    x = np.concatenate([np.full((1, 100), 1e30, np.float32), fx[5]["mel"].T, np.full((1, 100), 1e30, np.float32)])
    w, b = sd["encoder.0.0.weight"], sd["encoder.0.0.bias"]
    want, bound = R.conv(x, w, b, [(1, 5, 0)], 2, R.RELU_OUT)
    assert want[0].shape == (3, 32) and R.within(want[0].astype(np.float32), want[0], bound[0] + R.EPS * np.abs(want[0]))
    with np.errstate(all="ignore"):
        for variant in (dict(neighbour=True), dict(phase=1), dict(phase=-1), dict(reverse_taps=True), dict(swap_relu=True)):
            assert not R.within(R.conv(x, w, b, [(1, 5, 0)], 2, R.RELU_OUT, **variant)[0][0], want[0], bound[0]), variant
    r = np.ones((3, 32), np.float32)
    with_r, bound_r = R.conv(x, w, b, [(1, 5, 0)], 2, R.RESIDUAL, r)
    assert not R.within(R.conv(x, w, b, [(1, 5, 0)], 2, R.RESIDUAL, r, drop_residual=True)[0][0], with_r[0], bound_r[0])


def test_every_frame_of_the_fixture_is_decided():
    """From the float64 reference alone: with tau the fixture's own max |z32 - z64|, the margin of every frame's code over every
    other code exceeds 4 tau |e_best - e_j|_1 plus the search's rounding bound -- so the GPU tests may require the reference's
    code on EVERY frame and leave none out.  (This fixture: tau = 4.0e-7.)"""
    fx = R.fixture()
    t = R.tau(fx)
    assert 0 < t < 1e-5
    assert R.undecided(fx) == []
    assert sum(R.code_count(T) for T in R.FRAMES) == 56


# ----------------------------------------------------------------------------------------------------------- host side
def test_the_checkpoint_loader_holds_the_state_dict_against_the_config(tmp_path):
    from indextts.utils.checkpoint import check_dvae, load_dvae
    from indextts.utils.config import Config
    sd = state_dict()
    check_dvae(sd, VQ_SMALL)
    for change, what in ((dict(hidden_dim=64), "encoder.0.0.weight has the shape"), (dict(num_tokens=8192), "codebook.embed has the shape"),
                         (dict(num_resnet_blocks=2), "encoder.4.weight is missing"), (dict(num_resnet_blocks=4), "is missing"),
                         (dict(channels=80), "encoder.0.0.weight"), (dict(codebook_dim=64), "codebook.embed"),
                         (dict(positional_dims=2), "positional_dims 1"), (dict(num_layers=3), "num_layers 2")):
        with pytest.raises(ValueError, match=what):
            check_dvae(sd, dict(VQ_SMALL, **change))
    path = str(tmp_path / "dvae.pth")
    torch.save(dict(sd, **{"decoder.0.weight": torch.zeros(2, 2, 1)}), path)
    cfg = Config(dict(vqvae=VQ_SMALL, dvae_checkpoint="dvae.pth"))
    got = load_dvae(cfg, str(tmp_path))
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert sorted(load_dvae(cfg, "", path)) == sorted(sd)
    with pytest.raises(ValueError, match="codebook.embed has the shape"):
        load_dvae(Config(dict(vqvae=dict(VQ_SMALL, num_tokens=8192), dvae_checkpoint="dvae.pth")), str(tmp_path))
    with pytest.raises(ValueError, match="no vqvae block"):
        load_dvae(Config(dict(dvae_checkpoint="dvae.pth")), str(tmp_path))
    with pytest.raises(ValueError, match="no dvae_checkpoint"):
        load_dvae(Config(dict(vqvae=VQ_SMALL)), str(tmp_path))


def test_extract_codes_round_trip_on_a_host_stand_in(tmp_path):
    """extract_codes with the front-end and the engine replaced by host stand-ins: the files it writes load with np.load into the
    shapes and dtypes the reference's dataset expects ([1, T2] int64 codes, [1, 100, T] fp32 mels), in batches."""
    from indextts.infer import IndexTTS
    from indextts.vqvae import code_count, encoder_forward, nearest_code
    sd = state_dict()
    tts = object.__new__(IndexTTS)
    tts.device = torch.device("cpu")
    frames = {"a.wav": 37, "b.wav": 5, "c.wav": 160}
    batches = []

    class HostEngine:
        def encode(self, mels):
            batches.append(len(mels))
            return [nearest_code(encoder_forward(sd, m), sd["codebook.embed"]) for m in mels]

    tts._codec = HostEngine()
    tts._decode = lambda path: (torch.zeros(1, 256 * frames[os.path.basename(path)]), 24000)
    tts.prompt_mels = lambda audios, srs=None: [torch.from_numpy(R.fixture()[a[0].shape[-1] // 256]["mel"])[None] for a in audios]
    lst = tmp_path / "list.txt"
    lst.write_text("a.wav\thello there\n\n" + str(tmp_path / "sub" / "b.wav") + "\t你好\nc.wav\t tabs\tinside \n", encoding="utf-8")
    out = str(tmp_path / "out")
    recs = tts.extract_codes(str(lst), out, batch_clips=2)
    assert batches == [2, 1] and [r["text"] for r in recs] == ["hello there", "你好", "tabs\tinside"]
    assert [r["audio"] for r in recs] == [str(tmp_path / "a.wav"), str(tmp_path / "sub" / "b.wav"), str(tmp_path / "c.wav")]
    lines = [json.loads(x) for x in open(os.path.join(out, "metadata.jsonl"), encoding="utf-8")]
    assert lines == recs and all(sorted(r) == ["audio", "codes", "duration", "mels", "text"] for r in recs)
    for r, T in zip(recs, (37, 5, 160)):
        codes, mels = np.load(r["codes"]), np.load(r["mels"])
        assert codes.dtype == np.int64 and codes.shape == (1, code_count(T)) and mels.dtype == np.float32 and mels.shape == (1, 100, T)
        assert np.array_equal(codes[0], R.fixture()[T]["codes"]) and np.array_equal(mels[0], R.fixture()[T]["mel"])
        assert r["duration"] == pytest.approx(256 * T / 24000)
        assert torch.LongTensor(codes).shape == (1, code_count(T)) and torch.FloatTensor(mels).shape == (1, 100, T)
    (tmp_path / "bad.txt").write_text("no tab here\n")
    with pytest.raises(ValueError, match="bad.txt:1: expected"):
        tts.extract_codes(str(tmp_path / "bad.txt"), out)


def test_the_command_line_and_the_surface():
    import inspect
    from indextts.infer import IndexTTS
    cli = open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "cli.py")).read()
    assert '"--extract-codes"' in cli and '"--out"' in cli and "extract_codes_main(argv)" in cli
    for name in ("load_tokenizer", "audio_codes", "synthesize_codes", "extract_codes"):
        assert callable(getattr(IndexTTS, name))
    assert list(inspect.signature(IndexTTS.synthesize_codes).parameters)[:4] == ["self", "cond_mel", "text_token_rows", "code_rows"]
    tts = object.__new__(IndexTTS)
    with pytest.raises(ValueError, match="2 code rows for 1 texts"):
        tts.synthesize_codes(None, [torch.tensor([1])], [torch.tensor([1]), torch.tensor([2])])
