"""The voice pool on the host (no GPU): the residency policy, where a slot's image lies in the packed bank weight (against the header's
layout restated in numpy), voice-aware admission of fed items, the checks an engine with a pool makes before any launch, and the ABI,
which the pool leaves as it was."""
from types import SimpleNamespace

import numpy as np
import pytest

from indextts.gpt import voice_pool as vp


# ---------------------------------------------------------------------------------------------------------- residency
def test_hits_keep_their_slot_and_misses_take_empty_slots_then_the_lru_unpinned_one():
    r = vp.Residency(3)
    assert r.resident() == [None, None, None]
    assert r.acquire([3, 1]) == [(0, 3), (1, 1)]
    assert r.acquire([1, 4]) == [(2, 4)] and r.resident() == [3, 1, 4]          # a hit keeps its slot, the miss takes the empty one
    assert r.acquire([3]) == []                                                 # (3 is now the most recently used)
    assert r.acquire([7]) == [(1, 7)] and r.resident() == [3, 7, 4]             # LRU: 1 and 4 were last used together, lower slot first
    assert r.acquire([8, 3]) == [(2, 8)] and r.resident() == [3, 7, 8]          # 3 is wanted: never its own victim
    assert (r.loads, r.evictions, r.hits) == (5, 2, 3)


def test_pinned_voices_are_never_evicted_and_pins_stack():
    r = vp.Residency(2)
    r.acquire([0, 1])
    r.pin([0])
    r.pin([0])
    assert r.acquire([2]) == [(1, 2)]
    r.unpin([0])
    assert r.acquire([3]) == [(1, 3)] and r.resident() == [0, 3]                # one pin is left on 0
    r.pin([3])
    with pytest.raises(ValueError, match="0 slots are empty and 0 unpinned"):
        r.acquire([4])
    assert r.resident() == [0, 3]                                               # a refused acquire changes nothing
    r.unpin([0])
    assert r.acquire([4]) == [(0, 4)]
    with pytest.raises(ValueError, match="holds no pin"):
        r.unpin([0])


def test_more_distinct_voices_than_slots_raise_naming_the_counts():
    r = vp.Residency(3)
    with pytest.raises(ValueError, match="4 distinct voices.*3 slots"):
        r.acquire([0, 1, 2, 3])
    assert r.acquire([0, 1, 0, 2, 1]) == [(0, 0), (1, 1), (2, 2)]               # repeats are one voice
    r.pin([0, 1])
    with pytest.raises(ValueError, match="2 voices to page in"):
        r.acquire([5, 6])
    assert r.resident() == [0, 1, 2]


def test_remove_frees_the_slot_and_refuses_a_pinned_voice():
    pool = object.__new__(vp.VoicePool)                                          # the bookkeeping of remove(): no device storage
    pool._row, pool._free_rows = {0: 0, 1: 1, 2: 2}, []
    import weakref
    pool._residencies = weakref.WeakSet()
    r = vp.Residency(2)
    pool._residencies.add(r)
    r.acquire([0, 2])
    r.pin([2])
    with pytest.raises(ValueError, match="pinned"):
        pool.remove(2)
    assert pool.alive(2) and r.resident() == [0, 2]
    pool.remove(0)
    assert not pool.alive(0) and r.resident() == [None, 2] and len(pool) == 2
    with pytest.raises(ValueError, match="no voice 0"):
        pool.remove(0)
    r.unpin([2])
    pool.remove(2)
    assert r.resident() == [None, None]


# ---------------------------------------------------------------------------------------------------------- image span
def packed_rows_of(K, N, itemsize):
    """The header's packed weight layout over a logical [K][N] matrix, restated: the array of the packed buffer's ELEMENTS, each
    holding the logical row k it stores.  block(nt, ks) at (nt * KT + ks) KiB; inside, lane (g << 4) | c owns E elements
    W[ks * KS + g * E + e][nt * 16 + c]."""
    KS, E = (16, 4) if itemsize == 4 else (32, 8)
    KT, NT = K // KS, N // 16
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    nt, c, ks, g, e = n // 16, n % 16, k // KS, (k % KS) // E, k % E
    at = (nt * KT + ks) * (1024 // itemsize) + ((g << 4) | c) * E + e
    out = np.full(NT * KT * 1024 // itemsize, -1, dtype=np.int32)
    out[at.ravel()] = k.ravel()
    assert (out >= 0).all()
    return out


@pytest.mark.parametrize("itemsize", [2, 4])
@pytest.mark.parametrize("K,N", [(64, 64), (1280, 3840), (64, 3840), (1280, 64)])
@pytest.mark.parametrize("S,rp", [(4, 16), (3, 16), (2, 48)])
def test_a_slots_span_covers_exactly_its_rows_of_every_column_tile(itemsize, K, N, S, rp):
    """(4, 16): even and odd slots -- the halves of a 16-bit block; (3, 16): S * rp = 48 is no multiple of 32, the padding unit is
    never touched; (2, 48): a run that crosses blocks."""
    from indextts import _native as nat
    Kx = nat.lora_kx(S, rp)
    rows = packed_rows_of(K + Kx, N, itemsize)
    touched = np.zeros(rows.size, dtype=bool)
    for slot in range(S):
        NT, stride, off, run = vp.span(K, N, Kx, slot, rp, itemsize)
        assert NT == N // 16 and stride * NT == rows.size * itemsize and off % itemsize == 0 and run == rp * 16 * itemsize
        idx = (np.arange(NT)[:, None] * stride + off + np.arange(0, run, itemsize)[None]) // itemsize
        got = rows[idx]
        lo = K + slot * rp
        assert got.min() == lo and got.max() == lo + rp - 1                     # nothing but the slot's rows ...
        assert idx.size == rp * N and not touched[idx].any()                    # ... and all N columns of each of them, once
        assert all((got[t] == got[0]).all() for t in range(NT))                 # every column tile alike
        touched[idx] = True
    assert set(np.unique(rows[touched])) == set(range(K, K + S * rp))           # base rows and the padding unit stay as they are
    with pytest.raises(ValueError):
        vp.span(K, N, Kx, S if S * rp == Kx else Kx // rp, rp, itemsize)        # one past the last slot that fits


# ---------------------------------------------------------------------------------------------------------- admission
def test_admission_keeps_the_order_and_the_first_item_without_a_slot_blocks_the_later_ones():
    r = vp.Residency(2)
    r.acquire([0, 1])
    r.pin([0])                                                                   # one active row speaks with voice 0
    assert vp.admit_voices(r, [[0], [2], [3], [0]]) == 2                         # 3 finds no slot -- and the [0] behind it waits too
    assert vp.admit_voices(r, [[1, 2], [0]]) == 0                                # a two-voice mix beside a pinned voice: nothing passes it
    assert vp.admit_voices(r, [[], [0], [5], []]) == 4                           # the base voice needs no slot
    r.unpin([0])
    for voices in ([7], [8, 9], []):                                             # nothing pinned: an item alone always fits
        assert vp.admit_voices(r, [voices]) == 1
    assert vp.admit_voices(r, [[8, 9], [8], [9, 8], [4]]) == 3
    assert r.resident() == [0, 1]                                                # admission is a question: nothing moved


def pool_engine(slots, alive):
    from indextts.gpt.engine import GPTEngine
    eng = object.__new__(GPTEngine)
    eng.bank = SimpleNamespace(n=slots, rp=16, Kx=32 * ((slots * 16 + 31) // 32), sig=(slots, 16, ()),
                               pool=SimpleNamespace(alive=lambda v: v in alive), res=vp.Residency(slots), deferrals=0)
    return eng


def test_an_engine_with_a_pool_checks_voice_ids_against_the_pool():
    eng = pool_engine(2, {0, 1, 2, 5, 40})
    assert eng._row_adapters([40, -1, 5, 40], 4) == [40, -1, 5, 40]              # ids beyond the slots: pool voices
    assert eng.check_adapter_mix([{5: .7, 0: .3}, 40, None], 3, queue=True) == [((0, .3), (5, .7)), ((40, 1.0),), ()]
    with pytest.raises(ValueError, match="not"):
        eng._row_adapters([3], 1)                                                # never added / removed
    with pytest.raises(ValueError, match="voices of the pool"):
        eng.check_adapter_mix([{0: .5, 4: .5}], 1)
    with pytest.raises(ValueError, match="cannot be resident in the pool's 2 slots"):
        eng.check_adapter_mix([{0: .3, 1: .3, 2: .4}], 1)                        # a mix wider than S
    with pytest.raises(ValueError, match="3 distinct voices.*2 slots"):
        eng._voices([0, 1, 2], None, 3)                                          # one batch ...
    assert eng._voices([0, 1, 2], None, 3, queue=True)[0] == [0, 1, 2]           # ... but a queue's utterances take turns
    with pytest.raises(ValueError, match="3 distinct voices.*2 slots"):
        eng._voices(None, [0, {1: .5, 2: .5}], 2)
    assert eng._voices(None, [0, {1: .5, 2: .5}], 2, queue=True)[1] == [((0, 1.0),), ((1, .5), (2, .5))]


def test_slot_translation_names_slots_and_keeps_the_base_voice():
    eng = pool_engine(3, set(range(50)))
    eng._page_in = lambda loads: paged.extend(loads)
    paged = []
    assert eng._slots([33, -1, 36, 33], None) == ([0, -1, 1, 0], None) and paged == [(0, 33), (1, 36)]
    held = []
    assert eng._slots(None, [((2, .3), (36, .7)), ()], pin=held) == (None, [((1, .7), (2, .3)), ()])
    assert held == [2, 36] and paged[2:] == [(2, 2)] and eng.pool_resident() == [33, 36, 2]
    eng.bank.res.pin([33])
    with pytest.raises(ValueError, match="1 voices to page in"):
        eng._slots([7], None)                                                    # every slot holds a pinned voice
    eng.bank.res.unpin(held + [33])
    assert eng._slots([7], None) == ([0], None)                                  # ... and the least recently used one goes first
    assert eng.pool_stats() == {"loads": 4, "hits": 1, "evictions": 1, "deferrals": 0}


# ---------------------------------------------------------------------------------------------------------- ABI
def test_the_pool_adds_no_symbol():
    from indextts import _native as nat
    assert len(nat.EXPORTED_SYMBOLS) == 47 and nat.lib().itts_abi_version() == 10


# ---------------------------------------------------------------------------------------------------------- the loop's bookkeeping
class _Loop:
    """GPTEngine.decode_refill_chunks over a bare engine whose device work is stubbed (staged=False, contiguous cache): the host
    bookkeeping runs as it is -- feed, voice admission, held items, leftover, pins and guards.  A row's length is the stub's: row
    `tag` stops after LEN[tag] steps; a fed item carries its tag as its stop step."""
    LEN = {"r0": 12, "r1": 4, 10: 4, 11: 4, 12: 4, 13: 4}
    VOICE = {10: 2, 11: {3: .5, 4: .5}, 12: 0, 13: 1}

    def __init__(self, cap_s):
        import torch
        eng = self.eng = pool_engine(2, set(range(8)))
        self.res = eng.bank.res
        eng.device, eng._B, eng._S, eng._shared_prefix, eng._kv_rows, eng.kv, eng._cap_s = "cpu", 2, 10, None, None, None, cap_s
        eng._pad_host = [0, 0]
        eng.state, eng.kv_share = torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        eng.force_stop, eng.finished = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
        eng.history = torch.zeros(2, 256, dtype=torch.int32)
        eng.adapter_mix = eng._mix_records([()] * 2)
        eng._ids_host, eng._mix_host = None, [((0, 1.0),), ((1, 1.0),)]
        self.paged = []
        eng._page_in = self.paged.extend
        eng._slots(None, eng._mix_host, pin=[])                       # what prefill() leaves: the batch resident and pinned
        eng._prefill_pins = [0, 1]
        self.left, self.joins, self.queue = {0: self.LEN["r0"], 1: self.LEN["r1"]}, [], [10, 11, 12, 13]
        eng._graph_key = lambda *a, **k: "key"
        eng._sample = lambda *a, **k: None
        eng._poll = lambda: 0
        eng._token_loop, eng._stage, eng._join = self.steps, self.stage, self.join

    def steps(self, n, stop, *a, **k):
        for r in self.left:
            self.left[r] -= stop - n
            if self.left[r] <= 0:
                self.eng.finished[r] = 1
        return stop

    def stage(self, rows, prefixes, stops, n, mixes=None):
        return {"rows_h": list(rows), "tags": list(stops), "mix": mixes, "n": n}

    def join(self, st, sp, ev=None, row_sp=None, kernel=False):
        for r, tag, m in zip(st["rows_h"], st["tags"], st["mix"]):
            self.joins.append((st["n"], r, tag, m))
            self.left[r] = self.LEN[tag]
            self.eng.finished[r] = 0

    def feed(self, k):
        import torch
        take, self.queue = self.queue[:k], self.queue[k:]
        return [(torch.zeros(3, 4), tag, None, self.VOICE[tag]) for tag in take]

    def run(self):
        sp = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0)
        return self.eng.decode_refill_chunks(20, sp, self.feed, check_every=4, staged=False, voices=[0, 1], join="torch")


def test_the_loop_places_waiting_items_first_and_in_the_order_they_were_fed():
    lp = _Loop(cap_s=1000)
    seen = []
    for rec in lp.run():
        seen.append((rec["n"], sorted(lp.res.pins), sorted(lp.res.guards), [(r["utt"], r["stopped"]) for r in rec["rows"]]))
    # n = 5: row 1 (voice 1) has stopped and is still pinned at its poll; n = 9: item 10 (voice 2) took its slot and has stopped, and the
    # mix {3, 4} was fed beside the pinned voice 0: it waits, guarded; n = 13: row 0 ends; the mix enters ALONE (item 12, voice 0, fed
    # behind it, waits in turn) although two decode slots are free; then 12 and 13 enter together
    assert seen[0] == (5, [0, 1], [], [(0, False), (1, True)])
    assert seen[1] == (9, [0, 2], [], [(0, False), (2, True)])
    assert seen[2] == (13, [0], [3, 4], [(0, True)])
    assert seen[3] == (17, [3, 4], [0], [(3, True)])
    assert seen[4] == (21, [0, 1], [], [(4, True), (5, True)])
    assert [(n, tag) for n, _, tag, _ in lp.joins] == [(5, 10), (13, 11), (17, 12), (17, 13)]          # the order they were fed in
    assert [r for _, r, _, _ in lp.joins] == [1, 0, 0, 1]
    at = {v: s for s, v in enumerate(lp.res.resident())}
    assert lp.joins[-1][3] == ((at[1], 1.0),) and lp.joins[1][3] == ((0, .5), (1, .5))              # the rows' records name slots
    assert lp.eng.pool_stats()["deferrals"] == 2 and lp.eng.refill_leftover == []
    assert not lp.res.pins and not lp.res.guards and lp.eng._prefill_pins is None


def test_waiting_items_follow_the_refused_ones_into_the_leftover_in_feed_order():
    lp = _Loop(cap_s=45)              # positions for joins at n = 5 and n = 9 only: at n = 13 the loop can place nothing more
    polls = [rec["n"] for rec in lp.run()]
    assert polls == [5, 9, 13] and [tag for _, _, tag, _ in lp.joins] == [10]
    assert [it[1] for it in lp.eng.refill_leftover] == [11, 12]          # the mix that waited, then the item fed behind it
    assert all(len(it) == 4 and it[3] == _Loop.VOICE[it[1]] for it in lp.eng.refill_leftover)         # as they were fed
    assert not lp.res.pins and not lp.res.guards


def test_an_early_close_hands_the_waiting_item_back():
    lp = _Loop(cap_s=1000)
    loop = lp.run()
    for rec in loop:
        if rec["n"] == 13:
            assert sorted(lp.res.guards) == [3, 4] and lp.res.held(3) and not lp.res.pinned(3)
            with pytest.raises(ValueError, match="awaited"):
                lp.res.drop(3)                                               # a voice an item waits for stays in the pool
            break
    loop.close()
    assert [it[1] for it in lp.eng.refill_leftover] == [11] and not lp.res.pins and not lp.res.guards
