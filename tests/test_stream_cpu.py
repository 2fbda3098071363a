"""Streaming synthesis, the parts that need no GPU: the vocoder's halo is sufficient (through the fp32 oracle), the frame
planner partitions the utterance, and the refusals come before anything is launched."""
import types

import pytest
import torch

import synth
import weights
from oracle import bigvgan_ref

FRAMES = 96
HOP = 1024


def shipped_vocoder():
    from indextts.BigVGAN.models import BigVGAN
    from indextts.utils.config import Config
    return BigVGAN(Config(weights.reference_config()["bigvgan"]))


def small_generator():
    """The shipped generator's layers (rates, kernels, dilations: what the halo depends on) at 1/24 of its channels, a latent of
    8 columns and a speaker embedding of 4: (oracle weights, latent [1, FRAMES, 8], spk [1, 4, 1])."""
    import json
    import os
    shapes = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bigvgan_shapes.json")))
    small = {1280: 8, 512: 4}
    sd = {}
    for k, shp in shapes.items():
        if k.startswith("speaker_encoder."):
            continue
        shp = tuple(small.get(v, v // 24 if v >= 24 else v) for v in shp)
        try:
            sd[k] = synth.bigvgan_param(k, shp)
        except KeyError:
            pass                                    # the filters: deterministic buffers, the oracle builds them
    W = bigvgan_ref.Weights(sd)
    lat = torch.from_numpy(synth.uniform("stream.latent", (1, FRAMES, 8)))
    spk = torch.from_numpy(synth.uniform("stream.spk", (1, 4, 1)))
    return W, lat, spk


@pytest.fixture(scope="module")
def oracle_run():
    W, lat, spk = small_generator()
    with torch.no_grad():
        return W, lat, spk, bigvgan_ref.forward(lat, spk, W)[0, 0]


def test_shipped_halo_fits_the_trusted_window():
    left, right = shipped_vocoder().receptive_halo()
    assert (left, right) == (35, 35)                # the docstring's figure for the shipped configuration
    assert 0 < left <= 64 and 0 < right <= 64       # the 64-frame window the config-5 test relies on


@pytest.mark.parametrize("j", [0, 3, 48, 92, 95])
def test_halo_is_sufficient_through_the_oracle(oracle_run, j):
    """Adding 1.0 to latent frame j leaves every sample of the frames < j - right and > j + left EQUAL: a sample of frame t
    reads the latent frames [t - left, t + right] only."""
    W, lat, spk, base = oracle_run
    assert tuple(bigvgan_ref.UPSAMPLE_RATES) == tuple(shipped_vocoder().rates)     # the oracle runs the shipped layers
    left, right = shipped_vocoder().receptive_halo()
    moved = lat.clone()
    moved[0, j] += 1.0
    with torch.no_grad():
        out = bigvgan_ref.forward(moved, spk, W)[0, 0]
    assert out.shape == base.shape == (FRAMES * HOP,)
    lo, hi = max(0, j - right), min(FRAMES, j + left + 1)        # frames that may change
    assert torch.equal(out[: lo * HOP], base[: lo * HOP])
    assert torch.equal(out[hi * HOP:], base[hi * HOP:])
    assert not torch.equal(out[lo * HOP: hi * HOP], base[lo * HOP: hi * HOP])      # (the frame is not inert: the check is not vacuous)
    if j == 48:
        assert lo > 0 and hi < FRAMES                            # both sides are tested in the interior


def boundaries(T, chunk, right):
    """The (t0, t1) every boundary of an utterance of T frames emits: a boundary every `chunk` codes, the last at T."""
    from indextts.infer import IndexTTS
    out, emitted, k = [], 0, 0
    while True:
        k = min(k + chunk, T)
        final = k == T
        t0, t1 = IndexTTS.stream_plan(k, emitted, right, final)
        assert t0 == emitted and t1 >= t0
        if not final:
            assert t1 <= max(emitted, k - right)                 # the frames behind an emitted one exist
        if t1 > t0:
            out.append((t0, t1))
            emitted = t1
        if final:
            return out


@pytest.mark.parametrize("T,chunk,right", [(5, 8, 35), (20, 8, 35), (35, 8, 35), (36, 8, 35), (40, 8, 35), (64, 32, 35), (140, 32, 35),
                                          (96, 32, 35), (8, 8, 3), (24, 8, 3), (7, 8, 0), (16, 8, 0), (1, 1, 0), (0, 8, 35)])
def test_frame_planner_partitions_the_utterance(T, chunk, right):
    spans = boundaries(T, chunk, right)
    assert [a for a, _ in spans] == [0] * bool(spans) + [b for _, b in spans[:-1]]     # each begins where the last ended
    assert (spans[-1][1] if spans else 0) == T
    assert all(b > a for a, b in spans)
    if T > (right // chunk + 1) * chunk:
        assert len(spans) > 1                                    # audio leaves before the utterance ends


def test_refusals_come_before_anything_is_launched():
    from indextts.infer import IndexTTS
    nobody = types.SimpleNamespace()                 # no model, no device: the checks need neither
    text = torch.tensor([5, 6, 7])
    with pytest.raises(NotImplementedError):
        IndexTTS.stream_utterance(nobody, None, text, num_beams=3)
    with pytest.raises(ValueError):
        IndexTTS.stream_utterance(nobody, None, text, adapter_ids=[0, 1])
    with pytest.raises(ValueError):
        IndexTTS.stream_utterance(nobody, None, text, adapter_mix=[{0: 0.5}, {1: 0.5}])


class StubEngine:
    """infer_stream of an engine that needs no device: three chunks of known samples, or an error before / after the first."""

    def __init__(self):
        self.fail_at, self.calls, self.prompts = None, 0, []

    def infer_stream(self, prompt, text, limit, **kw):
        import os
        self.calls += 1
        self.prompts.append((prompt, os.path.exists(prompt)))
        assert kw["num_beams"] == 1 and kw["seed"] == 7
        for i in range(3):
            if self.fail_at == i:
                raise NotImplementedError("refused setting")
            yield 24000, torch.arange(4, dtype=torch.float32) + 100.0 * i - 0.75        # (truncated towards zero, as infer() writes)


def test_rest_stream_route_status_codes_bytes_and_cleanup(tmp_path):
    """/tts/stream over a stub engine: the body is the chunks' samples as little-endian int16; what fails before the first chunk
    answers 500 as /tts does, what fails after it ends the body; the engine lock is free again after each of them (the next
    request is served); an uploaded prompt's file is gone when the request is over."""
    import os

    import numpy as np
    from starlette.testclient import TestClient

    import api as itts_api
    tmp = str(tmp_path)
    prompt = os.path.join(tmp, "p.wav")
    open(prompt, "wb").write(b"RIFF")
    eng = StubEngine()
    app = itts_api.create_app(eng, model_dir=tmp, config_path=os.path.join(tmp, "config.yaml"), output_dir=os.path.join(tmp, "out"))
    c = TestClient(app)
    body = dict(text="hello", prompt_audio_path=prompt, seed=7)
    want = np.concatenate([np.arange(4, dtype=np.float32) + 100.0 * i - 0.75 for i in range(3)]).astype("<i2").tobytes()
    r = c.post("/tts/stream", json=body)
    assert r.status_code == 200 and r.content == want and r.headers["x-seed"] == "7"
    assert r.headers["content-type"].startswith("audio/L16") and "rate=24000" in r.headers["content-type"]
    eng.fail_at = 0
    r = c.post("/tts/stream", json=body)
    assert r.status_code == 500 and "refused setting" in r.text
    eng.fail_at = 2
    r = c.post("/tts/stream", json=body)
    assert r.status_code == 200 and r.content == want[: 2 * 8]            # the body ends early
    eng.fail_at = None
    r = c.post("/tts/stream", files={"prompt_audio": ("voice.wav", b"RIFFdata")}, data=dict(text="hello", seed="7"))
    assert r.status_code == 200 and r.content == want
    up, existed = eng.prompts[-1]
    assert existed and up.endswith(".wav") and not os.path.exists(up)     # the worker removed the upload
    assert c.post("/tts/stream", json=dict(text="hello")).status_code == 400
    assert c.post("/tts/stream", json=dict(text="hello", prompt_audio_path=os.path.join(tmp, "nope.wav"))).status_code == 404
    assert eng.calls == 4
