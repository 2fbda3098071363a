"""The two kernels of libindextts_audio.so against float64 on their fp32-rounded operands (tests/melfront_refs.py holds the
references, the derivation of the bounds and the negative controls; profiles/melfront_fp64.txt the measured ratios).

Resample: every output within (taps + 3) 2^-24 sum |kern| |xbar|; ratios 147->80, 2->1, 2->3, 147->160 and the 24 kHz channel
mean; C = 1, 2; N = orig k, orig k + 1 and 1000; a three-wave batch whose waves are bit-equal to themselves alone.
Log-mel: EVERY element in the linear domain, |exp(out) - max(mel64, 1e-7)| <= B + 2^-20 max(mel64, 1e-7); N = 513, 768, 4095, 4096,
4352; noise, a sine on a bin centre, zeros (exactly log(1e-7) in fp32), an impulse at either end; a batch of three lengths, every
prompt bit-equal to itself alone."""
import numpy as np
import pytest
import torch

import melfront_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from indextts.utils.audio_engine import PromptAudioEngine
    return PromptAudioEngine(DEV)


def run_resample(eng, waves, sr):
    """itta_resample alone over `waves` (planar fp32 arrays of one rate) in ONE launch -> their outputs."""
    from indextts import _native_audio as nata
    from indextts.utils.audio_engine import resample_plan
    rows, x_off, y_off = [], 0, 0
    orig, new, width, _ = resample_plan(sr)
    for w in waves:
        C, N = w.shape
        n_out = -(-new * N // orig)
        rows.append((x_off, y_off, C, N, n_out, 0))
        x_off, y_off = x_off + ((C * N + 3) & ~3), y_off + ((n_out + 3) & ~3)
    hx = torch.zeros(x_off)
    for w, r in zip(waves, rows):
        hx[r[0]:r[0] + w.size] = torch.tensor(w.reshape(-1))
    arr, raw = nata.seg_table(nata.WaveSeg, rows)
    x, y, segs = hx.to(DEV), torch.full((y_off,), float("nan"), device=DEV), raw.to(DEV)
    nata.resample(x, y, None if sr == 24000 else eng.taps(sr), orig, new, width, arr, segs)
    y = y.cpu().numpy()
    return [y[r[1]:r[1] + r[4]].copy() for r in rows]


def run_logmel(eng, signals):
    """itta_logmel alone over 24 kHz mono `signals` in ONE launch -> [100, T_i] arrays."""
    from indextts import _native_audio as nata
    rows, s_off, f_off = [], 0, 0
    for x in signals:
        T = 1 + x.size // 256
        rows.append((s_off, f_off, x.size, T))
        s_off, f_off = s_off + ((x.size + 3) & ~3), f_off + T
    hx = torch.zeros(s_off)
    for x, r in zip(signals, rows):
        hx[r[0]:r[0] + x.size] = torch.tensor(x)
    arr, raw = nata.seg_table(nata.MelSeg, rows)
    out = torch.full((100 * f_off,), float("nan"), device=DEV)
    nata.logmel(hx.to(DEV), out, eng.basis, eng.fb_t, eng.mel_rng, arr, raw.to(DEV))
    out = out.cpu().numpy()
    return [out[100 * r[1]:100 * (r[1] + r[3])].reshape(100, r[3]).copy() for r in rows]


@pytest.mark.parametrize("label", sorted(R.RATES))
def test_resample_within_the_dot_product_bound(eng, label):
    sr, worst = R.RATES[label], 0.0
    for lab, rate, C, N in R.resample_cases():
        if rate != sr:
            continue
        x, y, bound = R.resample_case(sr, C, N)
        got = run_resample(eng, [x], sr)[0]
        assert got.shape == y.shape and np.isfinite(got).all()
        r = R.resample_excess(got, y, bound)
        worst = max(worst, r)
        assert r <= 1.0, (label, C, N, r)
        assert np.array_equal(got, run_resample(eng, [x], sr)[0])                    # the same input gives the same bits
    print(f"resample {label}: worst |err| / bound {worst:.4f}")


@pytest.mark.parametrize("label", ["147->80", "2->3", "mean only"])
def test_resample_three_waves_in_one_launch_equal_the_waves_alone(eng, label):
    sr = R.RATES[label]
    cases = [c for c in R.resample_cases() if c[1] == sr]
    pick = [cases[0], cases[4], cases[2]]                                             # (C, N): (1, orig k), (2, orig k + 1), (1, 1000)
    assert len({(c[2], c[3]) for c in pick}) == 3 and len({c[3] for c in pick}) == 3
    waves = [R.resample_case(sr, C, N)[0] for _, _, C, N in pick]
    got = run_resample(eng, waves, sr)
    for w, g, (_, _, C, N) in zip(waves, got, pick):
        _, y, bound = R.resample_case(sr, C, N)
        assert R.resample_excess(g, y, bound) <= 1.0
        assert np.array_equal(g, run_resample(eng, [w], sr)[0]), (label, C, N)


@pytest.mark.parametrize("kind", R.MEL_SIGNALS)
def test_logmel_every_element_within_the_linear_bound(eng, kind):
    worst = 0.0
    for N in R.MEL_LENGTHS:
        x, mel, B = R.mel_case(kind, N)
        out = run_logmel(eng, [x])[0]
        assert out.shape == mel.shape == (100, 1 + N // 256) and np.isfinite(out).all()
        r = R.mel_excess(out, mel, B)
        worst = max(worst, r)
        assert r <= 1.0, (kind, N, r)
        if kind == "zeros":
            assert (out == np.float32(np.log(np.float64(np.float32(1e-7))))).all()
    print(f"log-mel {kind}: worst |exp(out) - max(mel64, 1e-7)| / (B + 2^-20 max(mel64, 1e-7)) {worst:.4f}")


def test_logmel_batch_of_three_lengths_is_bit_equal_to_each_alone(eng):
    sigs = [R.mel_case("noise", 4352)[0], R.mel_case("sine", 513)[0], R.mel_case("noise", 4095)[0]]
    together = run_logmel(eng, sigs)
    for x, got in zip(sigs, together):
        assert np.array_equal(got, run_logmel(eng, [x])[0])
    assert np.array_equal(run_logmel(eng, sigs[::-1])[2], together[0])               # nor does the order in the batch matter
    for (kind, N), got in zip((("noise", 4352), ("sine", 513), ("noise", 4095)), together):
        _, mel, B = R.mel_case(kind, N)
        assert R.mel_excess(got, mel, B) <= 1.0


def test_engine_chain_equals_the_two_launches(eng):
    """PromptAudioEngine.mel of a stereo 44.1 kHz wave and a mono 16 kHz one = resample, then log-mel, of each alone."""
    a, b = R.wave(2, 6000, 1), R.wave(1, 3000, 2)
    n0 = eng.launches
    mels = eng.mel([a, torch.from_numpy(b[0])], [44100, 16000])
    assert eng.launches == n0 + 3                                                     # one resample per rate, one log-mel
    for w, sr, m in ((a, 44100, mels[0]), (b, 16000, mels[1])):
        y = run_resample(eng, [w], sr)[0]
        want = run_logmel(eng, [y])[0]
        assert m.shape == (1, 100, 1 + y.size // 256) and m.is_cuda and m.dtype == torch.float32
        assert np.array_equal(m[0].cpu().numpy(), want)
    eng.forget()
    assert eng._bufs == {} and torch.equal(eng.mel([a], [44100])[0], mels[0])
