"""tests/select_dist.py and tests/select_dist_sets.py on the host: select_ref's sampler and beam step, driven over the draw sets of
tests/test_select_dist_gpu.py, stay inside every law and stream threshold for the committed seeds, and every negative control -- a
wrong law, or a stream with a counter or key word lost -- lands at least ten times over its threshold on the same counts.  Also
the pieces the shortcut through select_ref rests on: the chi-square quantile against tabulated values, the vectorised Philox
against select_ref's, the step-function lookup against select_ref.sample_case over whole launches."""
import numpy as np
import pytest

from tests import select_dist as D
from tests import select_dist_sets as S
from tests import select_ref as R

LAW_SETS = ("plain", "top-k", "top-p", "pool>64")


def report(checks):
    """Prints every check; returns the worst statistic / threshold of the laws and streams and the least of the controls."""
    worst, least = 0.0, np.inf
    for c in checks:
        print(S.line(c))
        if c[1].startswith("control"):
            least = min(least, c[2] / c[3])
        else:
            worst = max(worst, c[2] / c[3])
    return worst, least


def test_quantile_against_tables():
    """Upper critical values of chi-square as every table prints them (to the table's digits), and the survival function back."""
    for dof, q, x in ((1, 0.05, 3.841), (10, 0.01, 23.209), (100, 0.001, 149.449)):
        assert abs(D.chi2_isf(q, dof) - x) < 6e-4, (dof, q, D.chi2_isf(q, dof))
        assert abs(D.chi2_sf(D.chi2_isf(q, dof), dof) / q - 1) < 1e-8
    # dof = 2 is closed form: P(chi2 > x) = exp(-x / 2); the threshold itself
    assert abs(D.threshold(2) - 2 * np.log(1e9)) < 1e-6
    assert abs(D.gammq(0.5, 2.0) - 0.04550026389635842) < 1e-14           # erfc(sqrt(2)): the two-sigma tail
    t = [D.threshold(d) for d in (1, 15, 225, 1000)]
    assert all(a < b for a, b in zip(t, t[1:])) and 37.3 < t[0] < 37.4    # (6.1 sigma)^2


def test_philox_vectorised_is_select_refs():
    rng = np.random.default_rng(7)
    w = rng.integers(0, 2 ** 32, size=(300, 6), dtype=np.uint64)
    w[:8] = [[0] * 6, [R.M32] * 6, [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1]]
    got = D.philox_x0(*w.T)
    assert got.tolist() == [R.philox4x32_10(r[:4], r[4:])[0] for r in w.tolist()]
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0))[0] == 0x6627E8D5            # Random123's known-answer vectors
    assert R.philox4x32_10((R.M32,) * 4, (R.M32,) * 2)[0] == 0x408F276D
    for seed, s4, s5 in ((S.SEED + 1, R.M32, 0), (2 ** 64 - 1, 1, 0), (5, 7, 9), (2 ** 63, 0, 2 ** 31)):
        assert D.key_words(seed, s4, s5) == R.philox_key(seed, s4, s5)
        assert D.key_words(seed, s4, s5, "carry-dropped") == R.philox_key(seed, s4, s5, rules=("seed-carry-dropped",))
    k3, k2, k0 = (D.key_words(S.NIB_KEYS[k][0], *S.NIB_KEYS[k][1]) for k in ("K3", "K2", "K0"))
    assert k3 == k2 and D.key_words(S.NIB_KEYS["K3"][0], *S.NIB_KEYS["K3"][1], "carry-dropped") == k0 != k3
    assert D.key_words(S.NIB_KEYS["K2"][0], 0, 0, "seed-high-dropped") == k0


@pytest.mark.parametrize("name", LAW_SETS + ("nib K3",))
def test_lookup_is_select_ref(name):
    """One launch of the set through select_ref.sample_case, row by row (the first 768 rows: the counter word is the row), against
    the step-function lookup: tokens, history, finished, state.  The decisions that do not depend on u clear select_ref's budget, and
    the law keeps the ids select_ref keeps."""
    s = S.sampler_sets()[name]
    launch = {"plain": 3, "top-k": 11, "top-p": 0, "pool>64": 12, "nib K3": 15}[name]
    n = 768
    c = S.as_case(name, launch)
    c.update(lg=c["lg"][:n], hist=c["hist"][:n], finished=c["finished"][:n])
    want = R.sample_case(c)
    e = S.expected(name)
    assert want["tokens"] == e["tokens"][launch, :n].tolist()
    later = e["history"][:n].copy()
    for i in range(launch + 1, S.STEPS):
        if s["step0"] + i < S.CAP:
            later[:, s["step0"] + i] = s["hist"][s["group"][:n], s["step0"] + i]
    assert np.array_equal(want["history"], later)
    assert np.array_equal(want["finished"], e["finished"][:n]) and want["state"][2] == 0
    assert want["state"][0] == s["step0"] + launch + 1 and want["state"][1] == 100 + launch + 1
    for g in range(s["G"]):
        r = R.sample_row(s["lg"][g], S.penalty_ids(s, g), s["st"]["rep"], s["st"]["temp"], s["st"]["top_k"], s["st"]["top_p"], True, np.float32(0))
        assert r["margin"] > 1.0, (name, g, r["margin"])
        p = D.law(s["lg"][g], S.penalty_ids(s, g), s["st"])
        assert sorted(np.nonzero(p > 0)[0].tolist()) == sorted(r["kept"].tolist()), (name, g)
        first, kept = S.tables(name)[g]
        assert (np.diff(first) > 0).all() and first[-1] < 2 ** 24, (name, g, "a kept token no u reaches")


def test_sampler_sets_hold_their_laws_and_controls_do_not():
    checks = []
    for name in LAW_SETS:
        checks += S.law_checks(name, S.expected(name)["tokens"])
    worst, least = report(checks)
    assert worst < 1.0 and least >= 10.0, (worst, least)


def test_rows_set_holds_its_laws():
    e, s = S.expected_rows(), S.rows_set()
    a, b = S.TWINS
    assert s["seeds"][a] == s["seeds"][b] and np.array_equal(e["tokens"][:, a], e["tokens"][:, b])
    worst, _ = report(S.rows_law_checks(e["tokens"], controls=False))   # (a third of the draws per law: the controls are sized above)
    assert worst < 1.0, worst


def test_streams_are_independent_and_slips_are_not():
    nib = {k: S.nibbles_of(S.expected("nib " + k)["tokens"]) for k in S.NIB_KEYS}
    assert np.array_equal(nib["K3"], nib["K2"])                      # the key is the 64-bit sum: two ways to the same key
    for k in S.NIB_KEYS:
        assert np.array_equal(nib[k], D.nibble(S.expected("nib " + k)["u24"])), "a nibble row's token is floor(16 u)"
    worst, least = report(S.stream_checks(nib) + S.stream_controls(nib))
    assert worst < 1.0 and least >= 10.0, (worst, least)


def test_beam_set_holds_its_laws():
    c, want = S.beam_set(), S.expected_beam()
    assert want["margin"] > 1.0, want["margin"]
    assert want["arms"] >= {"b:fast", "b:top_p=1", "b:step0"} and not want["done"].any()
    tied = np.asarray(want["tokens"]).reshape(S.BEAM_B, 2)[c["kind"] == 2]
    b = np.arange(S.BEAM_B)[c["kind"] == 2]
    a, r = D.without_replacement_ranks(D.beam_u24(b, 0, 0, c["seed"], c["s45"]), D.beam_u24(b, 0, 1, c["seed"], c["s45"]))
    assert (S.beam_draws(want["tokens"])[0] == a).all() and (S.beam_draws(want["tokens"])[1] == r).all() and tied.shape[0] == 1024
    for L in S.beam_laws():
        assert abs(L["out_pair"].sum() - 1) < 1e-12 and abs(L["pair"].sum() - 1) < 1e-12 and (L["p"] > 0).sum() == 8
    worst, least = report(S.beam_checks(want["tokens"]) + S.beam_controls(want["tokens"]))
    assert worst < 1.0 and least >= 10.0, (worst, least)
