"""ConditionerEngine.batch: N prompts of different lengths in one pass of the 72 launches (gpt/conditioner.py), synthetic weights.

  accuracy   every row against this package's functional fp32 form of that prompt alone, at the bound test_frontend_gpu.py holds
             the single-prompt engine to (max-abs < 1e-2, RMS < 2e-3)
  spread     every row against the SINGLE-prompt engine (the yardstick; not bit-equal: the skinny GEMM's plan and the split of
             embed.out depend on the row count).  Measured on an MI355X: see SPREAD_MEASURED and profiles/prompt_batch.txt
  isolation  the other prompts replaced by noise of 10 x the amplitude: the unchanged prompt's latents keep their bits
  graph      a captured pass replays to the bits of the eager call; 72 launches for 4 prompts"""
import os

import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMES = [35, 36, 67, 120, 437]
# max |batched - single-prompt engine| over the five prompts above, measured on an MI355X (profiles/prompt_batch.txt); the
# assertion is 2 x that, rounded up to one digit
SPREAD_MEASURED = 2.463e-3
SPREAD_BOUND = 5e-3


@pytest.fixture(scope="module")
def model():
    from indextts.gpt.model import UnifiedVoice
    m = UnifiedVoice(**dict(weights.reference_config()["gpt"], layers=2))
    m.load_state_dict(weights.gpt_state_dict(2))
    return m.to(DEV).to(torch.bfloat16)


def mels_of(frames, tag="in.cond_mel"):
    """fp32 [T, 100] prompts, each its own draw"""
    return [torch.from_numpy(synth.uniform(f"{tag}.{i}", (1, 100, T), -6.0, 2.0)).to(DEV)[0].t().contiguous()
            for i, T in enumerate(frames)]


@pytest.fixture(scope="module")
def batched(model):
    """(mels, conds of ConditionerEngine.batch over them): computed once, shared, never written"""
    mels = mels_of(FRAMES)
    return mels, model.conditioner().batch(mels).clone()


def test_batch_matches_functional_fp32_of_each_prompt_alone(model, batched):
    mels, got = batched
    assert got.shape == (len(FRAMES), 32, 1280) and torch.isfinite(got).all()
    os.environ["ITTS_NATIVE_CONDITIONER"] = "0"
    try:
        ref = torch.cat([model.get_conditioning(m.t()[None], None) for m in mels], 0)
    finally:
        del os.environ["ITTS_NATIVE_CONDITIONER"]
    for i, T in enumerate(FRAMES):
        err = (got[i] - ref[i]).abs()
        print(f"frames {T}: max-abs {err.max().item():.3e} rms {err.pow(2).mean().sqrt().item():.3e}")
        assert err.max().item() < 1e-2 and err.pow(2).mean().sqrt().item() < 2e-3, (T, err.max().item())


def test_batch_spread_against_the_single_prompt_engine(model, batched):
    mels, got = batched
    eng = model.conditioner()
    worst = 0.0
    for i, m in enumerate(mels):
        one = eng(m).clone()
        e = (got[i] - one).abs().max().item()
        print(f"frames {FRAMES[i]}: max |batched - single| = {e:.3e}")
        worst = max(worst, e)
    print(f"spread max-abs {worst:.3e}")
    assert worst < SPREAD_BOUND, worst


def test_padded_batch_through_get_conditioning(model, batched):
    """UnifiedVoice.get_conditioning(mel [B, 100, Tmax], lengths): a 16-bit model conditions each prompt on its first
    cond_mel_lengths[b] frames, as if alone -- whatever the padding holds."""
    mels, got = batched
    tmax = max(FRAMES)
    mel = torch.full((len(FRAMES), 100, tmax), 50.0, device=DEV)
    for i, m in enumerate(mels):
        mel[i, :, : m.shape[0]] = m.t()
    out = model.get_conditioning(mel, torch.tensor(FRAMES, device=DEV))
    assert torch.equal(out, got)
    with pytest.raises(ValueError):
        model.get_conditioning(mel, torch.tensor([tmax + 1] * len(FRAMES)))


def test_a_prompt_does_not_see_its_neighbours(model, batched):
    """Same lengths, every OTHER prompt replaced by different noise at 10 x the amplitude: fails if a tap, a key or a statistic
    crosses a segment boundary."""
    mels, got = batched
    eng = model.conditioner()
    loud = [m * 10.0 for m in mels_of(FRAMES, tag="in.other_mel")]
    for keep in range(len(FRAMES)):
        mixed = [mels[i] if i == keep else loud[i] for i in range(len(FRAMES))]
        out = eng.batch(mixed)
        assert torch.equal(out[keep], got[keep]), keep
        assert not torch.equal(out[(keep + 1) % len(FRAMES)], got[(keep + 1) % len(FRAMES)])


def test_graph_replay_and_launch_count(model):
    eng = model.conditioner()
    mels = mels_of([35, 120, 36, 67])
    eager = eng.batch(mels).clone()
    assert eng.launches == 72                       # 3 + 9 * 6 + 2 + 6 * 2 + 1, whatever N: four single passes are 4 x 72
    static = [m.clone() for m in mels]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.batch(static)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # the table is device data of the buffers, not of the graph: other prompts of the same lengths replay through the same graph
    other = mels_of([35, 120, 36, 67], tag="in.other_mel")
    ref = eng.batch(other).clone()
    for s, o in zip(static, other):
        s.copy_(o)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    n = len(eng._bufs)
    eng.forget()
    assert len(eng._bufs) < n


def test_unretained_passes_keep_a_bounded_number_of_buffer_sets(model, batched):
    """batch(retain=False), what the prompt-list path of IndexTTS runs: every ordered tuple of lengths is a new key, the engine
    keeps at most MAX_UNRETAINED_SETS of them, and the latents are those of the retained pass bit for bit."""
    mels, got = batched
    eng = model.conditioner()
    eng.forget()
    order = [[0, 1, 2], [2, 1, 0], [1, 0, 2], [2, 0, 1], [0, 2, 1], [1, 2, 0], [0, 1, 2]]
    for o in order:
        out = eng.batch([mels[i].t().contiguous().t() for i in o], retain=False)     # views, as the public path passes them
        assert len(eng._bufs) <= eng.MAX_UNRETAINED_SETS
        assert out.shape[0] == 3 and torch.isfinite(out).all()
    # same tuple, retained and unretained: the same bits (and the retained set stays)
    ref = eng.batch([mels[i] for i in (0, 1, 2)]).clone()
    again = eng.batch([mels[i] for i in (0, 1, 2)], retain=False).clone()
    assert torch.equal(ref, again)
    for o in order[1:4]:
        eng.batch([mels[i] for i in o], retain=False)
    assert len(eng._bufs) == 1 + eng.MAX_UNRETAINED_SETS
    assert torch.equal(eng.batch([mels[i] for i in (0, 1, 2)]), ref)
    eng.forget()
    assert len(eng._bufs) == 0
