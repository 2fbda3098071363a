"""tests/select_ref.py proved on the host, before a GPU sees it: the reference agrees with the oracles where they are off every
rounding edge, every case of the table clears its decision budget, the table reaches every arm (and says so case by case), every
mutant of the reference changes something the GPU test compares, and the Philox restatement reproduces the known answers."""
import os

import numpy as np
import pytest

from oracle import beam_ref, sampling_ref
from tests import select_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def sampler():
    cases = R.sampler_cases()
    return cases, [R.sample_case(c) for c in cases]


@pytest.fixture(scope="module")
def beam():
    cases = R.beam_cases()
    return cases, [R.beam_case(c) for c in cases]


# ------------------------------------------------------------------------------------------------------------ 1. the oracles
def test_sampler_reference_agrees_with_the_hf_fixture_and_the_oracle():
    """The rows of tests/golden/sampling.npz (transformers' own processors; penalty 10, temperature 0.8, top-k 30, top-p 0.8): same
    kept sets, scores to the fixture test's rtol, the oracle's tokens under 8 (row, step) counters, the greedy tokens."""
    g = np.load(os.path.join(G, "sampling.npz"))
    for b in range(g["logits"].shape[0]):
        for step in range(8):
            u = R.uniform((b, step, 0, 0), R.philox_key(1234, 0, 0))
            assert u == sampling_ref.uniform01(1234, b, step)
            r = R.sample_row(g["logits"][b], g["history"][b], 10.0, 0.8, 30, 0.8, True, u)
            want = g["after_topp"][b]
            assert np.array_equal(np.isfinite(r["dbg"]), np.isfinite(want))
            np.testing.assert_allclose(r["dbg"][np.isfinite(want)], want[np.isfinite(want)], rtol=1e-6)
            assert r["token"] == sampling_ref.pick(want, u) and r["margin"] > 1.0
        r = R.sample_row(g["logits"][b], g["history"][b], 10.0, 0.8, 30, 0.8, False, 0.0)
        assert np.array_equal(r["dbg"].view(np.uint32), g["after_penalty"][b].view(np.uint32))      # the penalty is exact-layer
        assert r["token"] == int(np.argmax(g["after_penalty"][b]))


def _case_from_oracle(ref, lg, sp, lp, cap=64):
    """The device state itts_beam_step would hold where oracle/beam_ref.BeamSearch `ref` stands (before its next step)."""
    B, nb, k = ref.B, ref.nb, ref.k
    c = R._b("trajectory", lg, nb, set(), cap=cap, step=k, rep=sp["repetition_penalty"], temp=sp["temperature"], top_k=sp["top_k"],
             top_p=sp["top_p"], do_sample=sp["do_sample"], lp=lp, seed=ref.seed, eos=ref.eos, beam_scores=ref.scores.copy(), extra=(1, 8192),
             done=[int(d) for d in ref.done])
    for b in range(B):
        for j in range(nb):
            c["hist"][k & 1, b * nb + j, :k] = ref.hist[b][j][ref.plen:]
        hy = ref.hyps[b].beams
        c["n_hyp"][b] = len(hy)
        c["hyp_score"][b, : len(hy)] = [s for s, _ in hy]
        c["worst"][b] = ref.hyps[b].worst
    return c


@pytest.mark.parametrize("do_sample,lp", [(True, 0.0), (False, 0.0), (True, 1.0)])
def test_beam_reference_agrees_with_the_oracle_on_the_existing_trajectory(do_sample, lp):
    """The trajectory of test_kernels_gpu.py::test_beam_step_matches_oracle, one reference step at a time from the oracle's state:
    same tokens, source rows, done flags, hypothesis counts; running scores within the existing test's tolerance."""
    B, nb, V, steps = 3, 3, 8194, 14
    sp = dict(do_sample=do_sample, top_k=30, top_p=0.8, temperature=1.0 if not do_sample else 0.9, repetition_penalty=10.0)
    rng = np.random.default_rng(11)
    ref = beam_ref.BeamSearch(B, nb, sp, [1] * 5 + [8192], eos=8193, length_penalty=lp, seed=77)
    for k in range(steps):
        lg = (rng.normal(size=(B * nb, V)) * 2.5).astype(np.float32)
        if k >= 5:
            lg[:, 8193] += 6.0 + k
        got = R.beam_case(_case_from_oracle(ref, lg, sp, lp))
        t_ref, s_ref = ref.step(lg)
        assert got["tokens"].tolist() == t_ref.tolist() and got["src"].tolist() == s_ref.tolist(), k
        assert [bool(x) for x in got["done"]] == ref.done and got["n_hyp"].tolist() == [len(h.beams) for h in ref.hyps], k
        live = [b for b in range(B) if not ref.done[b]]
        assert np.allclose(got["beam_scores"].reshape(B, nb)[live], ref.scores[live], rtol=1e-5, atol=1e-4)
        if ref.all_done():
            break
    assert k >= 6


# ------------------------------------------------------------------------------------------------------------ 2. margins
def test_every_case_clears_its_budget(sampler, beam):
    """A condition on the test DATA: no case is left out, a case on an edge gets another seed in the table."""
    for cases, refs in (sampler, beam):
        for c, r in zip(cases, refs):
            assert r["margin"] > 1.0, (c["name"], r["margin"])
    for c in sampler[0]:
        assert R.sample_case(c, no_advance=True)["margin"] > 1.0


# ------------------------------------------------------------------------------------------------------------ 3. arms
def test_every_case_takes_the_arms_written_next_to_it(sampler, beam):
    for cases, refs in (sampler, beam):
        for c, r in zip(cases, refs):
            assert r["arms"] == c["arms"], (c["name"], sorted(r["arms"] ^ c["arms"]))
            assert R.arms(c) == c["arms"]


def test_the_table_reaches_every_arm(sampler, beam):
    reached = set().union(*(c["arms"] for c in sampler[0] + beam[0]))
    assert reached == set(R.ARMS), sorted(reached ^ set(R.ARMS))
    assert len({c["name"] for c in sampler[0] + beam[0]}) == len(sampler[0] + beam[0])
    alone = {a: [c["name"] for c in sampler[0] + beam[0] if a in c["arms"]] for a in R.ARMS}
    for a, names in alone.items():
        if len(names) == 1:
            print(f"select | {a} | carried alone by: {names[0]}")
    # the cases the issue names by shape
    V = {c["lg"].shape[1] for c in sampler[0]}
    assert V >= {1, 2, 255, 256, 257, 1000, 8194, 8448} and {c["pad"] for c in sampler[0]} == {0, 3}
    assert {c["top_k"] for c in sampler[0]} >= {1, 2, 30, 64, 65, 256, 257, 1024}
    assert {c["top_p"] for c in sampler[0]} >= {1.0, 0.8, 0.3, 1e-6} and {c["temp"] for c in sampler[0]} >= {0.7, 1.3}
    assert {r["n"] for rs in sampler[1] for r in rs["rows"]} >= {64, 65}
    assert {c["nb"] for c in beam[0]} == {2, 3, 8} and {c["B"] for c in beam[0]} == {1, 3}
    assert {c["lg"].shape[1] for c in beam[0]} >= {50, 8194} and {c["top_k"] for c in beam[0] if c["do_sample"]} >= {1, 2, 30, 128}
    assert {c["lp"] for c in beam[0]} == {0.0, 1.0} and {bool(c["do_sample"]) for c in beam[0]} == {True, False}


def test_the_philox_cases_spread_over_the_candidates(sampler):
    """32 (seed, stream, step) triples on one fixed row: at least three distinct candidates, not only the first."""
    toks, first = [], None
    for c, r in zip(*sampler):
        if "philox" in c["name"]:
            toks += r["tokens"]
            first = int(r["rows"][0]["kept"][0])
    assert len(toks) == 32 and len(set(toks)) >= 3 and any(t != first for t in toks)


def test_the_overflow_case_is_flagged(sampler):
    c, r = next((c, r) for c, r in zip(*sampler) if "all equal" in c["name"])
    assert all(x["overflow"] and x["token"] is None and x["n"] == c["lg"].shape[1] for x in r["rows"])


def test_padding_columns_and_sentinels_are_in_the_table(sampler, beam):
    assert any(c["pad"] for c in beam[0]) and any(c["step"] >= c["hist"].shape[2] for c in beam[0])
    assert any(c["step"] > c["hist"].shape[1] for c in sampler[0])


# ------------------------------------------------------------------------------------------------------------ 4. mutants
def _differs(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if isinstance(x, list):
            if x != y:
                return True
        elif x.dtype.kind == "f":
            w = a.get(k + "_w")
            if w is None:
                if not np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y):
                    return True
            elif np.any(np.abs(x - y) > w + b[k + "_w"]):
                return True
        elif not np.array_equal(x, y):
            return True
    return False


SAMPLER_COMPARED = ("tokens", "history", "finished", "state", "dbg")
BEAM_COMPARED = ("tokens", "src", "done", "n_hyp", "hyp_len", "hyp_tok", "hist", "cand_n", "state", "beam_scores", "hyp_score", "worst")


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught_by_a_compared_quantity(sampler, beam, mutant):
    caught = [c["name"] for c, r in zip(*sampler) if _differs(r, R.sample_case(c, rules=(mutant,)), SAMPLER_COMPARED)]
    caught += [c["name"] for c, r in zip(*beam) if _differs(r, R.beam_case(c, rules=(mutant,)), BEAM_COMPARED)]
    print(f"select | mutant {mutant} | caught by {len(caught)} case(s), first: {caught[0] if caught else None}")
    assert caught, f"no case of the table tells the reference from its mutant '{mutant}'"


def test_the_mutant_list_is_the_issues():
    assert len(R.MUTANTS) == len(set(R.MUTANTS)) == 10


# ------------------------------------------------------------------------------------------------------------ 5. Philox
def test_philox_known_answers_and_the_oracles_streams():
    """Random123's known-answer vectors for philox4x32-10 (the ones tests/test_oracle_vs_golden.py holds the oracle to), the
    oracle's two uniform streams, and the key's 64-bit carry."""
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox4x32_10((M := 0xFFFFFFFF,) * 4, (M,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    for seed in (0, 1234, 2 ** 32 - 1, 2 ** 32 + 7, 2 ** 63 + 3):
        for row, step, draw in ((0, 0, 0), (7, 3, 5), (M, 1000, 15)):
            assert R.uniform((row, step, 0, 0), R.philox_key(seed, 0, 0)) == sampling_ref.uniform01(seed, row, step)
            assert R.uniform((row, step, draw, 0), R.philox_key(seed, 0, 0)) == beam_ref.uniform01(seed, row, step, draw)
    assert R.philox_key(2 ** 32 - 5, 9, 0) == (4, 1) and R.philox_key(2 ** 32 - 5, 9, 0, ("seed-carry-dropped",)) == (4, 0)
    assert R.philox_key(2 ** 63 + 3, M, 0x7FFFFFFF) == (2, 0)             # wraps at 2^64
    assert R.philox_key(5, 0, 0) == R.philox_key(2, 3, 0) == R.philox_key(0, 5, 0)


def test_kv_rows_reference_is_the_documented_rule():
    for c in R.kv_cases():
        out = R.kv_rows_ref(c["tbl"], c["src"], c["k1"], c["P"])
        par = c["k1"] & 1
        assert np.array_equal(out[par ^ 1], c["tbl"][par ^ 1])
        assert np.array_equal(out[par][:, : c["P"]], c["tbl"][par ^ 1][c["src"]][:, : c["P"]])
        assert np.array_equal(out[par][:, c["P"]], np.arange(c["tbl"].shape[1])) and np.array_equal(out[par][:, c["P"] + 1:], c["tbl"][par][:, c["P"] + 1:])
    assert {(c["tbl"].shape[1], c["tbl"].shape[2]) for c in R.kv_cases()} >= {(2, 64), (24, 257)}
