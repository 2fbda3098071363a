"""itto_pcm_out on the GPU (libindextts_out.so, indextts/utils/pcm_out.py) against tests/pcm_out_refs.py:
`f32` held to float64 within the derived worst case of an fp32 fmaf chain, the integer encodings exact, rows isolated, streams
bit-equal to the one-shot encode, every negative control outside.

Shapes: N in {1, 2, width - 1, taps, 255, 256, 257, 1000, 4097} per rate, rates 8000 (new = 1), 16000, 48000 (orig = 1), 44100,
22050, 11025 (taps 348) and 24000 (the identity); Gaussian inputs at amplitude 8000 and one +-32767 square wave (with half-waves
beyond full scale) for the clamp.  A rate's rows go through the engine ONCE per encoding, as one ragged batch, and are kept."""
import functools

import numpy as np
import pytest
import torch

import pcm_out_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 2.0 ** -15


@functools.lru_cache(maxsize=None)
def engine():
    from indextts.utils.pcm_out import PcmOutEngine
    return PcmOutEngine(DEV)


def fmt(rate, enc):
    from indextts.utils.pcm_out import OutputFormat
    return OutputFormat(rate, enc)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rows_of(rate):
    """(kind, N) of the rate's rows: every length, then the square wave."""
    return [("gauss", n) for n in R.lengths(rate)] + [("square", 1000)]


@functools.lru_cache(maxsize=None)
def batch(rate, enc):
    """The rate's rows as ONE ragged launch in `enc`: a tuple of numpy arrays, computed once."""
    eng = engine()
    before = eng.launches
    outs = eng.encode([dev(R.case(rate, n, kind)[0]) for kind, n in rows_of(rate)], fmt(rate, enc))
    assert eng.launches == before + 1
    return tuple(o.cpu().numpy() for o in outs)


@pytest.mark.parametrize("rate", R.RATES)
def test_f32_is_within_the_fmaf_chain_bound_of_float64(rate):
    got = batch(rate, "f32")
    worst = 0.0
    for (kind, n), g in zip(rows_of(rate), got):
        x, v, b = R.case(rate, n, kind)
        assert g.dtype == np.float32 and g.shape == (R.out_len(n, rate),)
        r = R.excess(g, v, b, SCALE)
        worst = max(worst, r)
        assert r <= 1.0, (rate, kind, n, r)
    print(f"pcm_out f32 | rate {rate} | worst error / bound {worst:.3f}")
    # negative controls: the kernel's output against the neighbouring phase's taps and against taps laid one sample early
    x = R.case(rate, 1000)[0]
    g = got[[r for r in rows_of(rate)].index(("gauss", 1000))]
    if R.plan(rate)[1] > 1:
        assert R.excess(g, *R.ref64(x, rate, phase_shift=1), SCALE) > 1.0
    assert R.excess(g, *R.ref64(x, rate, width_off=1), SCALE) > 1.0


@pytest.mark.parametrize("rate", R.RATES)
def test_integer_encodings_are_exact(rate):
    f, p, mu, al = (batch(rate, e) for e in R.ENCODINGS)
    for (kind, n), gf, gp, gm, ga in zip(rows_of(rate), f, p, mu, al):
        v = (gf.astype(np.float32) * np.float32(2.0 ** 15))                # exact: the kernel's own v
        want = R.pcm16_of(v)
        assert gp.dtype == np.int16 and np.array_equal(gp, want), (rate, kind, n)
        assert gm.dtype == np.uint8 and np.array_equal(gm, R.mulaw_encode(gp)), (rate, kind, n)
        assert ga.dtype == np.uint8 and np.array_equal(ga, R.alaw_encode(gp)), (rate, kind, n)
        if kind == "gauss" and n == 1000:     # negative controls: rounding to nearest, mu-law with bias 128, A-law without its XOR
            assert not np.array_equal(gp, R.pcm16_of(v, "nearest"))
            assert not np.array_equal(gm, R.mulaw_encode(gp, bias=128)) and not np.array_equal(ga, R.alaw_encode(gp, xor=0))
        if kind == "square":
            assert np.abs(v).max() > 40000 and gp.max() == 32767 and gp.min() == -32767      # only the clamp brings these back


def test_every_int16_value_at_24_khz():
    """The exhaustive case: all 65 536 int16 values as fp32 through the identity rate, and the values just inside an integer
    (truncation, not rounding)."""
    s = np.arange(-32768, 32768, dtype=np.int64)
    x = dev(s.astype(np.float32))
    eng = engine()
    p, mu, al, f = (eng.encode([x], fmt(24000, e))[0].cpu().numpy() for e in ("pcm16", "mulaw", "alaw", "f32"))
    want = np.clip(s, -32767, 32767).astype(np.int16)
    assert np.array_equal(p, want) and np.array_equal(mu, R.mulaw_encode(want)) and np.array_equal(al, R.alaw_encode(want))
    assert np.array_equal(f, (s.astype(np.float64) / 32768.0).astype(np.float32))
    frac = dev((s[1:].astype(np.float32) - np.float32(0.25)))                  # k - 1/4 for every k: exact in fp32
    got = eng.encode([frac], fmt(24000, "pcm16"))[0].cpu().numpy()
    assert np.array_equal(got, np.trunc(np.clip(s[1:] - 0.25, -32767, 32767)).astype(np.int16))


def test_24_khz_pcm16_is_the_path_of_today():
    """clamp (as _vocode clamps), then numpy's astype on the host -- on samples of the vocoder's range and beyond."""
    x = np.concatenate([R.gauss(4097) * np.float32(3.0), R.square(1000)])
    today = np.clip(x, np.float32(-32767.0), np.float32(32767.0)).astype("int16")
    got = engine().encode([dev(x)], fmt(24000, "pcm16"))[0].cpu().numpy()
    assert np.array_equal(got, today)


@pytest.mark.parametrize("rate", R.RATES)
def test_a_row_in_a_batch_is_the_row_alone(rate):
    eng = engine()
    for enc in ("f32", "mulaw"):
        together = batch(rate, enc)
        for (kind, n), t in zip(rows_of(rate), together):
            alone = eng.encode([dev(R.case(rate, n, kind)[0])], fmt(rate, enc))[0].cpu().numpy()
            assert np.array_equal(alone, t), (rate, enc, kind, n)
    # five ragged rows, N = 1 among them and two rows short enough to share one workgroup-sized run, in another order and as views
    ns = [300, 1, 4097, 500, 257]
    big = dev(np.concatenate([R.gauss(n, seed=1) for n in ns]))
    cuts = np.cumsum([0] + ns)
    views = [big[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    got = eng.encode(views, fmt(rate, "pcm16"))
    for n, v, g in zip(ns, views, got):
        assert torch.equal(g, eng.encode([v.clone()], fmt(rate, "pcm16"))[0]), (rate, n)


@pytest.mark.parametrize("enc", R.ENCODINGS)
@pytest.mark.parametrize("rate", R.RATES)
def test_a_stream_is_the_one_shot_encode(rate, enc):
    eng, f = engine(), fmt(rate, enc)
    N = 1100
    x = dev(R.gauss(N, seed=2))
    whole = eng.encode([x], f)[0]
    for name, sizes in R.chunkings(N).items():
        st, at, parts = eng.stream(f), 0, []
        for i, c in enumerate(sizes):
            parts.append(st.push(x[at:at + c], last=i == len(sizes) - 1))
            at += c
            assert st.tail is None or st.tail.numel() <= st.plan.taps + st.plan.orig
        assert at == N and torch.equal(torch.cat(parts), whole), (rate, enc, name)
    if enc == "pcm16":
        # sample by sample, on an utterance shorter than the longest filter
        short = x[:200]
        st = eng.stream(f)
        parts = [st.push(short[i:i + 1], last=i == 199) for i in range(200)]
        assert torch.equal(torch.cat(parts), eng.encode([short], f)[0]), rate
        if rate != 24000:
            # negative control: a stream that drops its carried tail
            st, at, parts = eng.stream(f), 0, []
            sizes = R.chunkings(N)["256-aligned"]
            for i, c in enumerate(sizes):
                parts.append(st.push(x[at:at + c], last=i == len(sizes) - 1))
                at += c
                if st.tail is not None:
                    st.tail = torch.zeros_like(st.tail)
            assert not torch.equal(torch.cat(parts), whole), rate


@pytest.mark.parametrize("rate", R.RATES)
def test_push_many_interleaves_three_utterances_in_one_launch(rate):
    eng, f = engine(), fmt(rate, "mulaw")
    ns = [700, 1500, 1100]
    xs = [dev(R.gauss(n, seed=3 + i)) for i, n in enumerate(ns)]
    whole = eng.encode(xs, f)
    streams, at, parts = [eng.stream(f) for _ in ns], [0, 0, 0], [[], [], []]
    while any(a < n for a, n in zip(at, ns)):
        live = [i for i in range(3) if at[i] < ns[i]]
        step = [min(256 + 37 * i, ns[i] - at[i]) for i in live]
        before = eng.launches
        outs = eng.push_many([(streams[i], xs[i][at[i]:at[i] + c], at[i] + c == ns[i]) for i, c in zip(live, step)])
        assert eng.launches <= before + 1
        for i, c, o in zip(live, step, outs):
            parts[i].append(o)
            at[i] += c
    assert len({len(p) for p in parts}) == 3                                   # they end at different boundaries
    for i in range(3):
        assert torch.equal(torch.cat(parts[i]), whole[i]), (rate, i)
