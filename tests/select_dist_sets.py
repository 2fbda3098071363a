"""The draw sets of the distribution tests (tests/test_select_dist_cpu.py, tests/test_select_dist_gpu.py): what is launched, what
tests/select_ref.py says every launch must return, and the checks of tests/select_dist.py over the returned tokens.  Host only.

A SET is B = 4096 rows x 16 launches, state[0] stepping by one between launches (the kernels advance it themselves).  Rows of one
GROUP share a logits row and a history window, so the group has ONE law and 65 536 / groups draws from it.  A few rows of every
sampler set start finished: they must emit the stop token and are left out of the counts.

  plain      V 50, temperature 0.7, top_k = V, top_p 1                                  steps 0..15, history of 12 (written to 11)
  top-k      V 50, temperature 0.6, top_k 8                                              likewise
  top-p      V 50, temperature 0.9, top_k = V, top_p 0.8, penalty 1.3 over a window     steps 20..35: the window is the full 12-id
             of 12 ids and 5 extra ids (a repeat, an id in both, ids outside [0, V))     history, nothing is appended, the law holds
  pool>64    V 200, temperature 2.0, top_k 100: the lane-0 LDS arm of the running sums
  rows       itts_sample_rows, the three V 50 laws dealt per row; even rows draw under the call's seed with stream = row, odd rows
             under a 64-bit seed of their own with stream 0; rows 1 and 13 hold the same law and the same own seed.  The top-p rows
             run at row_step0 = -20 (their step is 20..35 while the others' is 0..15)
  nib K0..K4 nibble rows (16 ids tied, top_k 16) under five keys: seed s | s + 1 | s + 2^32 | s + 1 with state[4..5] =
             (0xFFFFFFFF, 0) | s + 1 with state[4..5] = (0, 1).  K3's key is s + 2^32: it must repeat K2 draw for draw; with the
             carry lost it would repeat K0
  beam       itts_beam_step, do_sample, B 2048 x 2 beams, V 50, top_k 8, penalty 1.2 on log-probabilities, step 0: even elements
             hold one of two laws, odd elements 16 tied ids (the stable sort then leaves the drawn candidates in draw order)

WHAT select_ref SAYS, 65 536 times.  select_ref.sample_row costs ~0.3 ms, so it is not called per draw: for fixed scores its pick is
a non-decreasing step function of u (`run > u` over a running sum), so `step_function` finds, by bisection over the 2^24 values u
can take, the first u of every step -- calling select_ref.sample_row each time -- and a draw's token is a table lookup.
tests/test_select_dist_cpu.py holds the lookup to select_ref.sample_case over whole launches, and the vectorised Philox of
select_dist to select_ref's.  A device token may differ from the lookup only where select_ref itself says the decision is inside
its expf budget (margin <= 1: some tens of the 2^24 values of u around each step, so a few dozen of 65 536 draws land there); it
must then be the neighbouring candidate (on an MI355X none did: profiles/select_dist.txt).  Nibble rows have budget 0 and the beam
set's seed is one under which every decision of select_ref.beam_case clears its budget: `==` throughout."""
import functools

import numpy as np

from tests import select_dist as D
from tests import select_ref as R

F32 = np.float32
B, STEPS, CAP = 4096, 16, 12
SEED = 0x5EED1234                      # high word 0: the keys K0..K4 line up as the docstring says
ROWS_SEED = 0x0123456789ABCDEF
OWN_SEED0, OWN_SEED_MUL = 0xC0FFEE0000000001, 0x9E3779B97F4A7C15
TWINS = (1, 13)
PRE_FINISHED = np.arange(B) % 512 == 5
BEAM_B, BEAM_NB, BEAM_SEED = 2048, 2, 0x2B7E151628AED2EA
NIB_IDS = np.array([0, 2, 5, 6, 9, 13, 17, 20, 22, 27, 31, 34, 38, 41, 44, 47])
NIB_KEYS = dict(K0=(SEED, (0, 0)), K1=(SEED + 1, (0, 0)), K2=(SEED + 2 ** 32, (0, 0)), K3=(SEED + 1, (R.M32, 0)), K4=(SEED + 1, (0, 1)))
LAW_CONTROLS = {"plain": ("temperature-ignored",), "top-k": ("temperature-ignored", "top_k+1", "top_k-1"),
                "top-p": ("penalty-ignored", "penalty-wrong-side", "top_p-keep+1", "top_p-keep-1", "not-renormalised"),
                "pool>64": ("temperature-ignored",)}


def _logits(groups, V, sigma, seed):
    return (np.random.default_rng(seed).standard_normal((groups, V)) * sigma).astype(F32)


@functools.lru_cache(maxsize=None)
def sampler_sets():
    """name -> dict(V, st (rep, temp, top_k, top_p), lg [G, V], hist [G, CAP], extra, step0, seed)."""
    S = {}
    none = np.full((4, CAP), -1, dtype=np.int32)
    S["plain"] = dict(V=50, st=dict(rep=1.0, temp=0.7, top_k=50, top_p=1.0), lg=_logits(4, 50, 1.0, 101), hist=none, extra=(), step0=0)
    S["top-k"] = dict(V=50, st=dict(rep=1.0, temp=0.6, top_k=8, top_p=1.0), lg=_logits(4, 50, 0.6, 102), hist=none, extra=(), step0=0)
    lg = _logits(4, 50, 2.0, 103)
    best = np.argsort(-lg, axis=1)
    hist = np.stack([[b[0], b[1], b[3], b[5], b[8], b[8], b[20], b[30], b[40], 50, -3, b[12]] for b in best]).astype(np.int32)
    S["top-p"] = dict(V=50, st=dict(rep=1.3, temp=0.9, top_k=50, top_p=0.8), lg=lg, hist=hist, extra=(2, 2, 64, -1, int(best[0, 0])), step0=20)
    S["pool>64"] = dict(V=200, st=dict(rep=1.0, temp=2.0, top_k=100, top_p=1.0), lg=_logits(2, 200, 1.0, 104), hist=none[:2], extra=(), step0=0)
    lg = np.full((1, 50), -4.0, dtype=F32)
    lg[0, NIB_IDS] = 1.0
    for name, (seed, s45) in NIB_KEYS.items():
        S["nib " + name] = dict(V=50, st=dict(rep=1.0, temp=0.7, top_k=16, top_p=1.0), lg=lg, hist=none[:1], extra=(), step0=0, seed=seed, s45=s45)
    for name, s in S.items():
        s.update(name=name, G=s["lg"].shape[0], stop=s["V"], seed=s.get("seed", SEED + 77 * len(name)), s45=s.get("s45", (0, 0)))
        s["group"] = np.arange(B) % s["G"]
        s["finished"] = (PRE_FINISHED & (not name.startswith("nib"))).astype(np.int32)
    return S


def penalty_ids(s, g):
    """What the law's history is for group g of set s: the extra ids and the window."""
    return np.concatenate([np.array(s["extra"], dtype=np.int64), s["hist"][g].astype(np.int64)])


# ------------------------------------------------------------------------------------------------------------------ select_ref, as a table
def _pick(lg, ids, st, m):
    r = R.sample_row(lg, ids, st["rep"], st["temp"], st["top_k"], st["top_p"], True, F32(m) * F32(2.0 ** -24))
    return int(np.nonzero(r["kept"] == r["token"])[0][0]), r


def step_function(lg, ids, st):
    """(first, kept): kept = select_ref's kept ids in its order; first[j] = the least m in [0, 2^24) at which select_ref.sample_row
    with u = m 2^-24 picks kept[j] or a later one (first[0] = 0)."""
    lo, hi = 0, 2 ** 24 - 1
    plo, r = _pick(lg, ids, st, lo)
    phi, _ = _pick(lg, ids, st, hi)
    kept = r["kept"]
    first = np.zeros(kept.shape[0] + 1, dtype=np.int64)
    first[phi + 1:] = 2 ** 24                                        # never reached
    assert plo == 0
    stack = [(lo, hi, plo, phi)]
    while stack:
        lo, hi, plo, phi = stack.pop()
        if plo == phi:
            continue
        if hi == lo + 1:
            first[plo + 1: phi + 1] = hi
            continue
        mid = (lo + hi) // 2
        pm, _ = _pick(lg, ids, st, mid)
        assert plo <= pm <= phi, "select_ref's pick is not monotone in u"
        stack += [(lo, mid, plo, pm), (mid, hi, pm, phi)]
    return first[:-1], kept


@functools.lru_cache(maxsize=None)
def tables(name):
    s = sampler_sets()[name]
    return [step_function(s["lg"][g], penalty_ids(s, g), s["st"]) for g in range(s["G"])]


def lookup(tabs, group, u24):
    """Tokens of the draws u24 (any shape) of rows in `group` (broadcasts against u24)."""
    u24 = np.asarray(u24).astype(np.int64)
    tok = np.zeros(u24.shape, dtype=np.int64)
    group = np.broadcast_to(group, u24.shape)
    for g, (first, kept) in enumerate(tabs):
        sel = group == g
        tok[sel] = kept[np.searchsorted(first, u24[sel], side="right") - 1]
    return tok


def bookkeeping(tok, fin0, stop, step_of_row, hist0):
    """What a set leaves behind, from its tokens [STEPS, B]: finished rows emit the stop token; a row's token goes to its history at
    its own step while that is below the capacity.  step_of_row [STEPS, B].  Returns (tokens, history, finished)."""
    tok = np.where(fin0[None, :] != 0, stop, tok)
    hist = hist0.copy()
    for i in range(tok.shape[0]):
        w = step_of_row[i] < hist.shape[1]
        hist[np.nonzero(w)[0], step_of_row[i][w]] = tok[i][w]
    return tok, hist, fin0.copy()


@functools.lru_cache(maxsize=None)
def expected(name):
    """select_ref's answer for itts_sample over set `name`: dict(tokens [STEPS, B], history [B, CAP], finished [B], state [4], u24)."""
    s = sampler_sets()[name]
    steps = s["step0"] + np.arange(STEPS)
    k0, k1 = R.philox_key(s["seed"], *s["s45"])
    u24 = D.philox_x0(np.arange(B)[None, :], steps[:, None], 0, 0, k0, k1) >> np.uint32(8)
    tok, hist, fin = bookkeeping(lookup(tables(name), s["group"][None, :], u24), s["finished"], s["stop"],
                                 np.broadcast_to(steps[:, None], (STEPS, B)), s["hist"][s["group"]])
    return dict(tokens=tok, history=hist, finished=fin, state=[s["step0"] + STEPS, 100 + STEPS, 0, 0], u24=u24)


def as_case(name, launch):
    """Launch `launch` of a sampler set as a select_ref case (select_ref.sample_case), from the history the launches before it left."""
    s = sampler_sets()[name]
    e = expected(name)
    step = s["step0"] + launch
    hist = s["hist"][s["group"]].copy()
    for i in range(launch):
        if s["step0"] + i < CAP:
            hist[:, s["step0"] + i] = e["tokens"][i]
    st = s["st"]
    return dict(lg=s["lg"][s["group"]], hist=hist, step=step, pos=100 + launch, extra=np.array(s["extra"], dtype=np.int32), rep=st["rep"],
                temp=st["temp"], top_k=st["top_k"], top_p=st["top_p"], do_sample=True, seed=s["seed"], s45=s["s45"],
                finished=list(s["finished"]), force=None, stop=s["stop"])


# ------------------------------------------------------------------------------------------------------------------ the rows set
ROWS_LAWS = ("plain", "top-k", "top-p")


@functools.lru_cache(maxsize=None)
def rows_set():
    """itts_sample_rows over the three V = 50 laws.  Row r: law (r // 4) % 3, group r % 4."""
    S = sampler_sets()
    r = np.arange(B)
    law_of, group = (r // 4) % 3, r % 4
    seeds = [ROWS_SEED if i % 2 == 0 else (OWN_SEED0 + i * OWN_SEED_MUL) & (2 ** 64 - 1) for i in range(B)]
    seeds[TWINS[1]] = seeds[TWINS[0]]
    stream = np.where(r % 2 == 0, r, 0)
    assert law_of[TWINS[0]] == law_of[TWINS[1]] and group[TWINS[0]] == group[TWINS[1]] and len(set(seeds[1::2])) == B // 2 - 1
    recs = []
    for i in range(B):
        st = S[ROWS_LAWS[law_of[i]]]["st"]
        recs.append(dict(do_sample=True, temperature=st["temp"], top_k=st["top_k"], top_p=st["top_p"], repetition_penalty=st["rep"],
                         seed=seeds[i], stream=int(stream[i])))
    lg = np.stack([S[ROWS_LAWS[law_of[i]]]["lg"][group[i]] for i in range(B)])
    hist = np.stack([S[ROWS_LAWS[law_of[i]]]["hist"][group[i]] for i in range(B)])
    row_step0 = np.where(law_of == 2, -S["top-p"]["step0"], 0).astype(np.int32)
    return dict(name="rows", V=50, lg=lg, hist=hist, extra=S["top-p"]["extra"], recs=recs, seeds=seeds, stream=stream, law_of=law_of,
                group=group, row_step0=row_step0, stop=50, step0=0, s45=(0, 0), finished=PRE_FINISHED.astype(np.int32))


@functools.lru_cache(maxsize=None)
def expected_rows():
    s = rows_set()
    keys = np.array([R.philox_key(sd, *s["s45"]) for sd in s["seeds"]], dtype=np.uint64)
    step = np.arange(STEPS)[:, None] - s["row_step0"][None, :]
    u24 = D.philox_x0(s["stream"][None, :], step, 0, 0, keys[None, :, 0], keys[None, :, 1]) >> np.uint32(8)
    tok = np.zeros((STEPS, B), dtype=np.int64)
    for li, name in enumerate(ROWS_LAWS):
        sel = s["law_of"] == li
        tok[:, sel] = lookup(tables(name), s["group"][sel][None, :], u24[:, sel])
    tok, hist, fin = bookkeeping(tok, s["finished"], s["stop"], step, s["hist"])
    return dict(tokens=tok, history=hist, finished=fin, state=[STEPS, 100 + STEPS, 0, 0], u24=u24)


# ------------------------------------------------------------------------------------------------------------------ the beam set
BEAM_EXTRA = (3, 7, 11, 19, 60)


@functools.lru_cache(maxsize=None)
def beam_set():
    lg2 = _logits(2, 50, 0.8, 105)
    for row in lg2:                                                    # two of the penalised ids are among the best, the EOS is not
        o = np.argsort(-row)
        row[[3, o[0]]] = row[[o[0], 3]]
        o = np.argsort(-row)
        row[[7, o[3]]] = row[[o[3], 7]]
        row[49] = -10.0
    tied = np.full(50, -6.0, dtype=F32)
    tied[NIB_IDS] = 1.0
    b = np.arange(BEAM_B)
    kind = np.where(b % 2 == 1, 2, (b // 2) % 2)                       # 0 / 1: the two laws, 2: tied
    lg = np.stack([lg2[0], lg2[1], tied])[np.repeat(kind, BEAM_NB)]
    c = R._b("dist", lg, BEAM_NB, (), cap=8, step=0, rep=1.2, temp=0.9, top_k=8, top_p=1.0, do_sample=True, lp=0.0, seed=BEAM_SEED,
             extra=BEAM_EXTRA, eos=49)
    c.update(kind=kind, laws=lg2, st=dict(rep=1.2, temp=0.9, top_k=8, top_p=1.0))
    return c


@functools.lru_cache(maxsize=None)
def expected_beam():
    return R.beam_case(beam_set())


# ------------------------------------------------------------------------------------------------------------------ checks
def law_checks(name, tokens, controls=True):
    """[(set, what, statistic, threshold)] of a sampler set's tokens [STEPS, B] against the law, summed over its groups; then
    the negative controls: the same counts against each wrong law."""
    s = sampler_sets()[name]
    live = s["finished"] == 0
    out = []
    for what in (None,) + (LAW_CONTROLS[name] if controls else ()):
        stat, dof = 0.0, 0
        for g in range(s["G"]):
            counts = np.bincount(tokens[:, live & (s["group"] == g)].ravel(), minlength=s["V"] + 1)[: s["V"]]
            hist = penalty_ids(s, g)
            p = D.law(s["lg"][g], hist, s["st"]) if what is None else D.wrong_law(s["lg"][g], hist, s["st"], what)
            x, d = D.chi2_gof(counts, p)
            stat, dof = stat + x, dof + d
        out.append((name, "law" if what is None else "control " + what, stat, D.threshold(dof)))
    return out


def rows_law_checks(tokens, controls=True):
    s, S = rows_set(), sampler_sets()
    live = s["finished"] == 0
    out = []
    for li, name in enumerate(ROWS_LAWS):
        for what in (None,) + (LAW_CONTROLS[name] if controls else ()):
            stat, dof = 0.0, 0
            for g in range(4):
                counts = np.bincount(tokens[:, live & (s["law_of"] == li) & (s["group"] == g)].ravel(), minlength=51)[:50]
                hist = penalty_ids(S[name], g)
                p = D.law(S[name]["lg"][g], hist, S[name]["st"]) if what is None else D.wrong_law(S[name]["lg"][g], hist, S[name]["st"], what)
                x, d = D.chi2_gof(counts, p)
                stat, dof = stat + x, dof + d
            out.append(("rows " + name, "law" if what is None else "control " + what, stat, D.threshold(dof)))
    # the two kinds of stream hold the same laws: a law statistic per kind over all twelve (law, group) cells
    for kind, sel in (("call seed, stream = row", np.arange(B) % 2 == 0), ("own seed, stream 0", np.arange(B) % 2 == 1)):
        stat, dof = 0.0, 0
        for li, name in enumerate(ROWS_LAWS):
            for g in range(4):
                counts = np.bincount(tokens[:, live & sel & (s["law_of"] == li) & (s["group"] == g)].ravel(), minlength=51)[:50]
                x, d = D.chi2_gof(counts, D.law(S[name]["lg"][g], penalty_ids(S[name], g), S[name]["st"]))
                stat, dof = stat + x, dof + d
        out.append(("rows " + kind, "law", stat, D.threshold(dof)))
    return out


def nibbles_of(tokens):
    """Tokens of a nibble set -> floor(16 u); a token outside the 16 tied ids is a failure."""
    n = np.searchsorted(NIB_IDS, tokens)
    assert np.array_equal(NIB_IDS[np.minimum(n, 15)], tokens), "a nibble row drew a token outside its pool"
    return n


def _table(name, what, a, b, nb=16):
    x, d = D.chi2_table(a, b, 16, nb)
    return (name, what, x, D.threshold(d))


def stream_checks(nib):
    """nib: K0..K4 -> nibbles [STEPS, B].  The independence tables of the issue, each over disjoint pairs."""
    k0 = nib["K0"]
    edge = np.arange(255, B, 256)
    distinct = ("K0", "K1", "K2", "K4")                               # (K3 repeats K2)
    out = [_table("nib K0", "row r | row r + 1", k0[:, 0::2], k0[:, 1::2]),
           _table("nib K0", "step k | step k + 1", k0[0::2], k0[1::2]),
           _table("nib K0 K1", "seed s | s + 1", k0, nib["K1"]),
           _table("nib K0 K2", "seed s | s + 2^32", k0, nib["K2"]),
           _table("nib K3 K4", "state[4..5] (0xFFFFFFFF, 0) | (0, 1)", nib["K3"], nib["K4"]),
           _table("nib K3 K0", "the key past the carry | the key with the carry lost", nib["K3"], k0),
           _table("nib K0 K1 K2 K4", "rows 255 | 256, 511 | 512, ... 4095 | 0",
                  np.stack([nib[k][:, edge] for k in distinct]), np.stack([nib[k][:, (edge + 1) % B] for k in distinct]))]
    for k in NIB_KEYS:                                                 # and the nibbles themselves are uniform
        x, d = D.chi2_gof(np.bincount(nib[k].ravel(), minlength=16), np.full(16, 1 / 16))
        out.append(("nib " + k, "uniform", x, D.threshold(d)))
    return out


def stream_controls(nib):
    """One side from `nib` (the streams a slip leaves alone), the other what the partner stream draws under the slip."""
    rows, steps = np.arange(B)[None, :], np.arange(STEPS)[:, None]
    k0 = nib["K0"]

    def wrong(key, slip, r=rows, k=steps):
        seed, s45 = NIB_KEYS[key]
        return D.nibble(D.sampler_u24(r, k, seed, s45, slip))
    return [_table("nib K0", "control row word dropped: row 0 | row r", np.broadcast_to(k0[:, :1], (STEPS, B - 1)), wrong("K0", "row-dropped", r=rows[:, 1:])),
            _table("nib K0", "control step word dropped: step 0 | step k", np.broadcast_to(k0[:1], (STEPS - 1, B)), wrong("K0", "step-dropped", k=steps[1:])),
            _table("nib K0 K2", "control high seed word dropped: s | s + 2^32", k0, wrong("K2", "seed-high-dropped")),
            _table("nib K0 K3", "control state[5] carry dropped: s | s + 1 + 0xFFFFFFFF", k0, wrong("K3", "carry-dropped"))]


def beam_draws(tokens):
    """Tied elements of the beam set -> (first draw 0..15, rank of the second among the 15 left), from the emitted tokens of beams 0, 1."""
    c = beam_set()
    t = np.asarray(tokens).reshape(BEAM_B, BEAM_NB)[c["kind"] == 2]
    a, b = nibbles_of(t[:, 0]), nibbles_of(t[:, 1])
    assert (a != b).all(), "a candidate was drawn twice"
    return a, b - (b > a)


@functools.lru_cache(maxsize=None)
def beam_laws():
    c = beam_set()
    return [D.beam_law(c["laws"][g], BEAM_EXTRA, c["st"], BEAM_NB, eos=c["eos"]) for g in range(2)]


def beam_checks(tokens):
    c = beam_set()
    t = np.asarray(tokens).reshape(BEAM_B, BEAM_NB)
    out = []
    s1 = s2 = 0.0
    d1 = d2 = 0
    for g, L in enumerate(beam_laws()):
        tg = t[c["kind"] == g]
        x, d = D.chi2_gof(np.bincount(tg[:, 0], minlength=50)[:50], L["out_first"])
        s1, d1 = s1 + x, d1 + d
        x, d = D.chi2_gof(np.bincount(tg[:, 0] * 50 + tg[:, 1], minlength=2500)[:2500], L["out_pair"])
        s2, d2 = s2 + x, d2 + d
    out.append(("beam", "law of beam 0's token (best of the four drawn)", s1, D.threshold(d1)))
    out.append(("beam", "joint law of the tokens of beams 0 and 1", s2, D.threshold(d2)))
    a, r = beam_draws(tokens)
    x, d = D.chi2_gof(np.bincount(a, minlength=16), np.full(16, 1 / 16))
    out.append(("beam tied", "law of the first draw", x, D.threshold(d)))
    x, d = D.chi2_gof(np.bincount(a * 15 + r, minlength=240), np.full(240, 1 / 240))
    out.append(("beam tied", "joint law of the first two draws, without replacement", x, D.threshold(d)))
    out.append(_table("beam tied", "draw 0 | draw 1", a, r, nb=15))
    return out


def beam_controls(tokens):
    c = beam_set()
    b = np.arange(BEAM_B)[c["kind"] == 2]
    a, _ = beam_draws(tokens)
    _, r = D.without_replacement_ranks(D.beam_u24(b, 0, 0, c["seed"], c["s45"]), D.beam_u24(b, 0, 1, c["seed"], c["s45"], "draw-dropped"))
    out = [_table("beam tied", "control draw index dropped: draw 0 | draw 1", a, r, nb=15)]
    t = np.asarray(tokens).reshape(BEAM_B, BEAM_NB)
    # (the best two of four drawn from eight hardly move with the temperature or a ninth candidate at 512 elements a law: no
    # control that could not tell is kept)
    for what, st in (("penalty ignored", dict(c["st"], rep=1.0)),):
        stat, dof = 0.0, 0
        for g in range(2):
            tg = t[c["kind"] == g]
            x, d = D.chi2_gof(np.bincount(tg[:, 0] * 50 + tg[:, 1], minlength=2500)[:2500], D.beam_law(c["laws"][g], BEAM_EXTRA, st, BEAM_NB, eos=c["eos"])["out_pair"])
            stat, dof = stat + x, dof + d
        out.append(("beam", "control " + what + ": joint law of the tokens of beams 0 and 1", stat, D.threshold(dof)))
    return out


def line(check):
    name, what, stat, thr = check
    return f"select-dist | {name} | {what} | {stat:.4g} / {thr:.4g} = {stat / thr:.3g}"
