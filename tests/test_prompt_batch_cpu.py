"""Host side of the per-row voice prompts (no GPU): the row space and the segment tables of ConditionerEngine.batch, the table
checks of the three segmented entry points (refused before any launch), prompt deduplication and the argument checks of the
public interface."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_space_alignment_and_offsets():
    from indextts.gpt.conditioner import prompt_row_space, prompt_seg_records
    frames = [35, 36, 67, 120, 437, 3]
    sp = prompt_row_space(frames)
    assert sp["t"] == [(T - 3) // 2 + 1 for T in frames] == [17, 17, 33, 59, 218, 1]
    assert all(r % 16 == 0 for r in sp["row0"]) and sp["row0"] == [0, 32, 64, 112, 176, 400]
    assert sp["M"] == sum((t + 15) // 16 * 16 for t in sp["t"]) == 416
    assert sp["frame0"] == [0, 35, 71, 138, 258, 695] and sp["total_frames"] == sum(frames)
    # a 16-row tile holds rows of one prompt only
    owner = {}
    for p, (r0, t) in enumerate(zip(sp["row0"], sp["t"])):
        for r in range(r0, r0 + t):
            assert owner.setdefault(r // 16, p) == p
    recs = prompt_seg_records(sp, 32)
    assert recs["conv"][1] == recs["enc"][1] == 26 and recs["per"][1] == 6 * 32 // 16
    assert recs["conv"][0][2] == (64, 33, 71, 67) and recs["enc"][0][2] == (64, 33, 64, 33, 0, 0, 64)
    # the Perceiver: prompt p's 32 latent rows, then its context rows behind ALL latent rows
    assert recs["per"][0][2] == (64, 32, 64, 32, 6 * 32 + 64, 33, 64)
    with pytest.raises(ValueError):
        prompt_row_space([120, 2])
    with pytest.raises(ValueError):
        prompt_row_space([])


def test_segment_words():
    from indextts import _native as nat
    w = nat.seg_words([(0, 17, 0, 35), (32, 5, 35, 11)], 3)
    assert w.dtype == torch.int32 and w.tolist() == [0, 17, 0, 35, 0, 0, 0, 0, 32, 5, 35, 11, 0, 0, 0, 0, 0, 0, 1]
    assert nat.seg_words([(0, 5)], 2, tile_map=[0, -1]).tolist()[-2:] == [0, -1]
    with pytest.raises(ValueError):
        nat.seg_words([], 1)
    with pytest.raises(ValueError):
        nat.seg_words([(0, 5)], 2, tile_map=[0])


def test_abi_declares_and_exports_the_prompt_entry_points():
    from indextts import _native as nat
    L = nat.lib()
    main = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    declared = set(re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", txt))
    syms = ["itts_glu_dwconv_ln_silu_seg", "itts_mha_small_seg", "itts_subsample_conv_seg"]
    plain = ctypes.CDLL(nat.LIB_PATH)
    assert all(s_ in declared and hasattr(plain, s_) and s_ in nat.EXPORTED_SYMBOLS for s_ in syms)
    assert int(re.search(r"#define ITTS_SEG_WORDS (\d+)", txt).group(1)) == nat.SEG_WORDS
    assert ctypes.sizeof(nat.SegTableArgs) == 24 and ctypes.sizeof(nat.MhaArgs) == ctypes.sizeof(nat.MhaArgs())
    assert L.itts_abi_version() == int(re.search(r"#define ITTS_ABI_VERSION (\d+)", main).group(1))


def _tab(nat, recs, ntiles, tile_map=None):
    """a table whose 'device' copy is never read: every call below is refused before a launch"""
    words = nat.seg_words(recs, ntiles, tile_map)
    return words, nat.SegTableArgs(ctypes.c_void_p(0x1000), ctypes.c_void_p(words.data_ptr()), len(recs), ntiles)


BAD = [("a multiple of 16", [(0, 5, 0, 11), (24, 5, 11, 11)], None),
       ("overlap", [(0, 20, 0, 41), (16, 5, 41, 11)], None),
       ("length 0", [(0, 5, 0, 11), (16, 0, 11, 3)], None),
       ("tile map", [(0, 5, 0, 11), (16, 5, 11, 11)], [0, 0, -1]),
       ("no segment covers", [(0, 5, 0, 11)], [0, -1, 0]),
       ("ends past", [(0, 5, 0, 11), (32, 17, 11, 35)], [0, -1, 1])]


@pytest.mark.parametrize("what,recs,tmap", BAD)
def test_invalid_tables_are_refused_before_any_launch(what, recs, tmap):
    from indextts import _native as nat
    L = nat.lib()
    P = 0x1000
    keep, tab = _tab(nat, recs, 3, tmap)
    assert L.itts_subsample_conv_seg(P, P, P, P, ctypes.byref(tab), 64, 5, 8, nat.F16, None) == 1
    assert b"itts_subsample_conv_seg" in L.itts_last_error() and what.encode() in L.itts_last_error()
    assert L.itts_glu_dwconv_ln_silu_seg(P, P, P, P, P, P, ctypes.byref(tab), 128, 15, 3, 1e-5, nat.BF16, None) == 1
    assert what.encode() in L.itts_last_error()
    a = nat.MhaArgs()
    a.dtype, a.Tq, a.Tk, a.H = nat.F16, 48, 48, 2
    a.q = a.k = a.v = a.out = P
    a.q_stride = a.k_stride = a.v_stride = 384
    a.out_mtp = 3
    assert L.itts_mha_small_seg(ctypes.byref(a), ctypes.byref(tab), 0, None) == 1
    assert what.encode() in L.itts_last_error()


def test_ranges_of_a_valid_table_are_held_against_the_buffers():
    from indextts import _native as nat
    L = nat.lib()
    P = 0x1000
    # the frames of the second prompt end past the mel; the row count does not follow from the frame count
    for recs in ([(0, 5, 0, 11), (16, 5, 60, 11)], [(0, 6, 0, 11)]):
        keep, tab = _tab(nat, recs, 2 if len(recs) == 2 else 1)
        assert L.itts_subsample_conv_seg(P, P, P, P, ctypes.byref(tab), 64, 5, 8, nat.F16, None) == 1
    a = nat.MhaArgs()
    a.dtype, a.Tq, a.Tk, a.H = nat.F16, 32, 40, 2
    a.q = a.k = a.v = a.out = P
    a.q_stride = a.k_stride = a.v_stride = 384
    a.out_mtp = 2
    for rec, why in (((0, 17, 0, 17, 30, 11, 0), b"key rows"), ((0, 17, 0, 17, 0, 0, 24), b"output rows"), ((0, 17, 0, 17, 0, 0, 16), b"output rows"),
                     ((0, 17, 0, 0, 0, 0, 0), b"key rows")):
        keep, tab = _tab(nat, [rec], 2)
        assert L.itts_mha_small_seg(ctypes.byref(a), ctypes.byref(tab), 0, None) == 1 and why in L.itts_last_error()
    a.pos = a.bias_u = a.bias_v = P
    keep, tab = _tab(nat, [(0, 17, 0, 17, 0, 0, 0)], 2)
    assert L.itts_mha_small_seg(ctypes.byref(a), ctypes.byref(tab), 16, None) == 1 and b"pos holds 16" in L.itts_last_error()
    keep, tab = _tab(nat, [(0, 17)], 2)
    assert L.itts_glu_dwconv_ln_silu_seg(P, P, P, P, P, P, ctypes.byref(tab), 128, 15, 1, 1e-5, nat.BF16, None) == 1
    assert b"y_mtp" in L.itts_last_error()
    assert L.itts_glu_dwconv_ln_silu_seg(P, P, P, P, P, P, ctypes.byref(tab), 128, 15, 2, 1e-5, nat.F32, None) == 1


def test_prompt_deduplication():
    from indextts.infer import dedupe_prompts
    a, b, c = torch.zeros(1, 100, 40), torch.zeros(1, 100, 40), torch.zeros(1, 100, 55)
    uniq, idx = dedupe_prompts([a, b, a, c, b], 5)
    assert [id(u) for u in uniq] == [id(a), id(b), id(c)] and idx == [0, 1, 0, 2, 1]     # by identity: a and b hold equal values
    uniq, idx = dedupe_prompts([a, a, a], 3)
    assert len(uniq) == 1 and uniq[0] is a and idx == [0, 0, 0]
    with pytest.raises(ValueError, match="2 prompts for 3 utterances"):
        dedupe_prompts([a, b], 3)
    with pytest.raises(ValueError, match=r"\[1, n_mels, T\]"):
        dedupe_prompts([a, torch.zeros(100, 40)], 2)
    with pytest.raises(ValueError, match=r"\[1, n_mels, T\]"):
        dedupe_prompts([a, "prompt.wav"], 2)
    with pytest.raises(ValueError, match="mel bins"):
        dedupe_prompts([a, torch.zeros(1, 80, 40)], 2)


class _StubEngine:
    bank = None

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was reached: the arguments are checked before anything is launched")


class _StubGpt:
    engine = _StubEngine()

    def __getattr__(self, name):
        raise AssertionError(f"gpt.{name} was reached: the arguments are checked before anything is launched")


def _stub_tts():
    from indextts.infer import IndexTTS
    tts = IndexTTS.__new__(IndexTTS)
    tts._gpt = _StubGpt()
    return tts


def test_argument_checks_come_before_any_launch():
    tts = _stub_tts()
    a, b = torch.zeros(1, 100, 40), torch.zeros(1, 100, 55)
    texts = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
    for call in (tts.infer_batch, tts._batch_tokens):
        with pytest.raises(ValueError, match="3 prompts for 2 utterances"):
            call([a, b, a], texts, num_beams=1)
        with pytest.raises(NotImplementedError, match="beam search with a prompt per utterance"):
            call([a, b], texts, num_beams=3)
        with pytest.raises(NotImplementedError, match="beam search with a prompt per utterance"):
            call([a, b], texts)                                  # the default is the reference's num_beams = 3
    with pytest.raises(ValueError, match="1 prompts for 2 utterances"):
        tts.infer_queue([a], texts, num_beams=1)
    with pytest.raises(ValueError, match=r"\[1, n_mels, T\]"):
        tts.infer_queue([a, a[0]], texts, num_beams=1)
    # a list that names ONE prompt for every utterance is that prompt: the single-tensor path
    assert tts._check_prompts([a, a], 2, {"num_beams": 1}, "infer_batch") is a
    assert tts._check_prompts(a, 2, {"num_beams": 3}, "infer_batch") is a
    both = tts._check_prompts((a, b), 2, {"num_beams": 1}, "infer_batch")
    assert isinstance(both, list) and both[0] is a and both[1] is b


def test_unretained_buffer_sets_stay_bounded_over_many_length_tuples():
    """The public prompt-list path runs ConditionerEngine.batch(retain=False): however many distinct ordered tuples of lengths a
    service sees, a thread keeps at most MAX_UNRETAINED_SETS of those sets; sets a graph may replay into (retain=True) stay until
    forget().  Pure host: the bookkeeping of _keep over stand-in buffer sets."""
    import threading
    from indextts.gpt.conditioner import ConditionerEngine
    eng = ConditionerEngine.__new__(ConditionerEngine)
    eng._bufs, eng._unretained = {}, []
    me = threading.get_ident()
    cap = ConditionerEngine.MAX_UNRETAINED_SETS
    assert 1 <= cap <= 4
    lens = (120, 67, 151)
    n = 0
    for a in lens:                                    # 3 lengths only, yet 3^4 ordered tuples
        for b in lens:
            for c in lens:
                for d in lens:
                    key = ((a, b, c, d), 100, me)
                    eng._keep(key, dict(retained=False), False)
                    n += 1
                    assert len(eng._bufs) <= cap and key in eng._bufs        # the newest is always there
    assert n == 81 and len(eng._bufs) == cap
    # a retained set is not counted against the cap and survives any number of unretained ones
    held = ((1, 2), 100, me)
    eng._keep(held, dict(retained=True), True)
    other = ((9, 9), 100, me + 1)                     # another thread's set is not this thread's to drop
    eng._keep(other, dict(retained=False), False)
    for i in range(10):
        eng._keep(((300 + i,), 100, me), dict(retained=False), False)
    assert held in eng._bufs and other in eng._bufs and len(eng._bufs) == cap + 2
    # least recently USED goes first: touching the older set saves it
    if cap > 1:
        mine = [k for k in eng._unretained if k[2] == me]
        eng._keep(mine[0], eng._bufs[mine[0]], False)
        eng._keep(((999,), 100, me), dict(retained=False), False)
        assert mine[0] in eng._bufs and mine[1] not in eng._bufs
    # an unretained set that a caller now wants to capture over is promoted, and stays
    promoted = [k for k in eng._unretained if k[2] == me][-1]
    eng._bufs[promoted]["retained"] = True
    eng._keep(promoted, eng._bufs[promoted], True)
    for i in range(5):
        eng._keep(((500 + i,), 100, me), dict(retained=False), False)
    assert promoted in eng._bufs and held in eng._bufs
    eng.forget()
    assert list(eng._bufs) == [other] and eng._unretained == [other]


def test_latents_refuse_conds_that_fit_neither_one_nor_every_row():
    tts = _stub_tts()
    tts.device = "cpu"
    tts.reuse_prompt_kv = True
    with pytest.raises(ValueError, match="4 prompts for 2 rows"):
        tts._latents(torch.zeros(4, 32, 8), [torch.tensor([1]), torch.tensor([2])], [torch.tensor([3]), torch.tensor([4])])
    with pytest.raises(ValueError, match="4 prompts for 2 rows"):
        tts._latents(torch.zeros(4, 32, 8), [torch.tensor([1]), torch.tensor([2])], [torch.tensor([3]), torch.tensor([4])], reuse_prefix=True)
