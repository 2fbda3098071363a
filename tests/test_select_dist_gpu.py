"""itts_sample, itts_sample_rows and itts_beam_step (do_sample) held to the DISTRIBUTIONS they must draw from, over the draw sets
of tests/select_dist_sets.py: 4096 rows x 16 launches a set, every set launched once and kept.

  exactness at scale   every token of every launch is select_ref's (the step-function lookup; where select_ref says a draw's decision
                       lies inside its own expf budget the neighbouring candidate is accepted, and counted); the history holds what
                       was emitted, finished rows emit the stop token, state[0..3] counts the launches; nibble rows and the beam
                       step compare with `==`
  the law              Pearson chi-square of the device's counts against tests/select_dist.py's law, a second derivation
  the streams          16 x 16 independence tables over nibble rows: neighbouring rows, steps, seeds, keys across the carry
  the controls         the same device counts against each wrong law, the device's draws against each slipped stream: all at
                       least ten times over the threshold (nothing is launched again)
  no stray writes      sentinels behind the tokens, the history and every logits row keep their bytes

Every statistic must lie below the 1 - 1e-9 chi-square quantile of its degrees of freedom; the seeds are fixed.  One line per
check: `select-dist | set | statistic / threshold` (profiles/select_dist.txt)."""
import functools

import numpy as np
import pytest
import torch

from tests import select_dist as D
from tests import select_dist_sets as S
from tests import select_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 64
LAW_SETS = ("plain", "top-k", "top-p", "pool>64")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def guarded(a, fill, pad=0):
    """`a` [rows, n] on the device with `pad` columns of `fill` behind every row and TAIL elements of it behind the last: (the
    [rows, n] view, the whole buffer)."""
    rows, n = a.shape
    buf = np.full(rows * (n + pad) + TAIL, fill, dtype=a.dtype)
    buf[: rows * (n + pad)].reshape(rows, n + pad)[:, :n] = a
    whole = dev(buf)
    return whole[: rows * (n + pad)].view(rows, n + pad)[:, :n], whole


def untouched(whole, rows, n, pad, fill, what):
    got = whole.cpu().numpy()
    assert (got[rows * (n + pad):] == fill).all(), (what, "tail")
    if pad:
        assert (got[: rows * (n + pad)].reshape(rows, n + pad)[:, n:] == fill).all(), (what, "row padding")


def launch_set(s, rows):
    """The 16 launches of a sampler set (itts_sample, or itts_sample_rows when `rows`).  Returns dict(tokens [STEPS, B], history,
    finished, states [STEPS, 8]) after checking the sentinels."""
    from indextts import _native as nat
    V = s["V"]
    lg_rows = s["lg"] if rows else s["lg"][s["group"]]
    hist0 = s["hist"] if rows else s["hist"][s["group"]]
    lg, lg_whole = guarded(lg_rows.astype(np.float32), np.float32(1e30), pad=3)
    tokens, tok_whole = guarded(np.full((S.STEPS, S.B), -5, dtype=np.int32), np.int32(-5))
    history, hist_whole = guarded(hist0.astype(np.int32), np.int32(-77))
    finished = dev(s["finished"], np.int32)
    st = np.zeros(8, dtype=np.uint32)
    st[0], st[1], st[4], st[5] = s["step0"], 100, s["s45"][0], s["s45"][1]
    state = dev(st.view(np.int32))
    states = torch.zeros((S.STEPS, 8), dtype=torch.int32, device=DEV)
    extra = dev(np.array(s["extra"], dtype=np.int32)) if len(s["extra"]) else None
    if rows:
        recs = torch.from_numpy(nat.pack_sample_rows(s["recs"])).to(DEV)
        row_step0 = dev(s["row_step0"], np.int32)
    for i in range(S.STEPS):
        if rows:
            nat.sample_rows(lg, tokens[i], history, finished, state, extra, None, recs, s["stop"], None, no_advance=False, row_step0=row_step0)
        else:
            t = s["st"]
            nat.sample(lg, tokens[i], history, finished, state, extra, None, t["rep"], t["temp"], t["top_k"], t["top_p"], True, s["seed"],
                       s["stop"], None, no_advance=False)
        states[i].copy_(state)
    torch.cuda.synchronize()
    untouched(lg_whole, S.B, V, 3, np.float32(1e30), (s["name"], "logits"))
    untouched(tok_whole, S.STEPS, S.B, 0, -5, (s["name"], "tokens"))
    untouched(hist_whole, S.B, S.CAP, 0, -77, (s["name"], "history"))
    assert torch.equal(lg.cpu(), torch.from_numpy(lg_rows.astype(np.float32))), (s["name"], "logits changed")
    return dict(tokens=tokens.cpu().numpy().astype(np.int64), history=history.cpu().numpy(), finished=finished.cpu().numpy(),
                states=states.cpu().numpy())


@functools.lru_cache(maxsize=None)
def device_set(name):
    return launch_set(S.rows_set() if name == "rows" else S.sampler_sets()[name], rows=name == "rows")


def exact(name, got, want, row_law):
    """Assertion 1 for a sampler set.  row_law(b) -> the set of tests/select_dist_sets.sampler_sets whose law row b holds, and its group."""
    s = S.rows_set() if name == "rows" else S.sampler_sets()[name]
    diff = np.argwhere(got["tokens"] != want["tokens"])
    assert diff.shape[0] <= 256, (name, "tokens differ from select_ref's in", diff.shape[0], "draws; first", diff[:4].tolist())
    for i, b in diff.tolist():
        ls, g = row_law(b)
        t = ls["st"]
        r = R.sample_row(ls["lg"][g], S.penalty_ids(ls, g), t["rep"], t["temp"], t["top_k"], t["top_p"], True,
                         np.float32(want["u24"][i, b]) * np.float32(2.0 ** -24))
        pos = {int(tok): j for j, tok in enumerate(r["kept"])}
        near = int(got["tokens"][i, b]) in pos and abs(pos[int(got["tokens"][i, b])] - pos[r["token"]]) == 1
        assert s["finished"][b] == 0 and r["margin"] <= 1.0 and near, (name, "launch", i, "row", b, int(got["tokens"][i, b]), r["token"], r["margin"])
    print(f"select-dist | {name} | exact: {got['tokens'].size - diff.shape[0]} of {got['tokens'].size} tokens are select_ref's, "
          f"{diff.shape[0]} inside its expf budget took the neighbour")
    step = s["step0"] + np.arange(S.STEPS)[:, None] - (s["row_step0"][None, :] if name == "rows" else 0)
    hist0 = s["hist"] if name == "rows" else s["hist"][s["group"]]
    _, hist, fin = S.bookkeeping(got["tokens"], s["finished"], s["stop"], np.broadcast_to(step, (S.STEPS, S.B)), hist0)
    assert (got["tokens"][:, s["finished"] != 0] == s["stop"]).all(), (name, "a finished row drew")
    assert np.array_equal(got["history"], hist), (name, "history")
    assert np.array_equal(got["finished"], fin), (name, "finished")
    for i in range(S.STEPS):
        assert got["states"][i, :4].tolist() == [s["step0"] + i + 1, 100 + i + 1, 0, 0], (name, "state after launch", i, got["states"][i].tolist())
    assert got["states"][-1, :4].tolist() == want["state"]
    assert (got["states"][:, 4:6].astype(np.int64) & R.M32 == np.array(s["s45"])).all(), (name, "state[4..5]")


def judge(checks, controls=True):
    worst, least = 0.0, np.inf
    for c in checks:
        print(S.line(c))
        if c[1].startswith("control"):
            least = min(least, c[2] / c[3])
        else:
            worst = max(worst, c[2] / c[3])
    assert worst < 1.0, ("a statistic is over its threshold", worst)
    assert not controls or least >= 10.0, ("a control is not ten times over its threshold", least)


@pytest.mark.parametrize("name", LAW_SETS)
def test_sample_set(name):
    """itts_sample over one settings group: exact at B = 4096 over 16 steps, the device's counts under the law, the wrong laws not."""
    s = S.sampler_sets()[name]
    got = device_set(name)
    exact(name, got, S.expected(name), lambda b: (s, int(s["group"][b])))
    judge(S.law_checks(name, got["tokens"]))


def test_sample_rows_set():
    """itts_sample_rows with the settings dealt per row, call-seed and own-seed streams, a row step of its own for a third of the
    rows (a third of the draws per law: the controls are sized on the itts_sample sets and not repeated here).  Rows with the same own seed, stream 0, law and step draw the same token: the documented stream-0 identity."""
    s, S_ = S.rows_set(), S.sampler_sets()
    got = device_set("rows")
    exact("rows", got, S.expected_rows(), lambda b: (S_[S.ROWS_LAWS[s["law_of"][b]]], int(s["group"][b])))
    a, b = S.TWINS
    assert np.array_equal(got["tokens"][:, a], got["tokens"][:, b]) and len(set(got["tokens"][:, a].tolist())) > 1
    judge(S.rows_law_checks(got["tokens"], controls=False), controls=False)


def test_streams():
    """Nibble rows under the five keys: every token is floor(16 u) of select_ref's stream; rows, steps, seeds and keys are pairwise
    independent; a stream with the row, step, high seed word or carry lost is not."""
    nib = {}
    for k in S.NIB_KEYS:
        got, want = device_set("nib " + k), S.expected("nib " + k)
        assert np.array_equal(got["tokens"], want["tokens"]), ("nib " + k, np.argwhere(got["tokens"] != want["tokens"])[:4].tolist())
        exact("nib " + k, got, want, None)
        nib[k] = S.nibbles_of(got["tokens"])
    assert np.array_equal(nib["K3"], nib["K2"])                      # seed + state[4..5] is one 64-bit sum
    judge(S.stream_checks(nib) + S.stream_controls(nib))


@functools.lru_cache(maxsize=None)
def device_beam():
    from indextts import _native as nat
    c = S.beam_set()
    R_, V = c["lg"].shape
    i32 = dict(dtype=torch.int32, device=DEV)
    lg, lg_whole = guarded(c["lg"], np.float32(1e30), pad=3)
    tokens, tok_whole = guarded(np.full((1, R_), -5, dtype=np.int32), np.int32(-5))
    st = np.zeros(8, dtype=np.uint32)
    st[0], st[1], st[4], st[5] = c["step"], c["pos"], c["s45"][0], c["s45"][1]
    t = dict(tokens=tokens[0], src=torch.full((R_,), -5, **i32), beam_scores=dev(c["beam_scores"]), hist=dev(c["hist"]), hyp_score=dev(c["hyp_score"]),
             hyp_len=dev(c["hyp_len"]), hyp_tok=dev(c["hyp_tok"]), n_hyp=dev(c["n_hyp"]), worst=dev(c["worst"]), done=dev(c["done"]),
             state=dev(st.view(np.int32)))
    scratch = (torch.full((R_, 1024), 3.0, device=DEV), torch.full((R_, 1024), -1, **i32), torch.full((R_,), -1, **i32))
    nat.beam_step(lg, c["nb"], t["tokens"], t["src"], t["beam_scores"], t["hist"], t["hyp_score"], t["hyp_len"], t["hyp_tok"], t["n_hyp"],
                  t["worst"], t["done"], t["state"], dev(c["extra"]), c["rep"], c["temp"], c["top_k"], c["top_p"], c["do_sample"], c["lp"],
                  c["seed"], c["eos"], scratch=scratch)
    torch.cuda.synchronize()
    untouched(lg_whole, R_, V, 3, np.float32(1e30), ("beam", "logits"))
    untouched(tok_whole, 1, R_, 0, -5, ("beam", "tokens"))
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["cand_n"] = scratch[2].cpu().numpy()
    return out


def test_beam_sample_set():
    """One itts_beam_step launch, do_sample, 2048 elements x 2 beams from a fresh state: select_ref's outputs with `==` (scores within
    its budget), the emitted tokens under the beam law, the first two draws of the tied elements uniform without replacement and
    independent, and not so when the draw index is lost."""
    c, want, got = S.beam_set(), S.expected_beam(), device_beam()
    assert want["margin"] > 1.0
    assert got["cand_n"].tolist() == want["cand_n"].tolist()
    for k in ("tokens", "src", "done", "n_hyp", "hyp_len", "hyp_tok", "hist"):
        assert np.array_equal(got[k], want[k].reshape(got[k].shape)), ("beam", k, np.argwhere(got[k] != want[k].reshape(got[k].shape))[:4].tolist())
    assert got["state"][:4].tolist() == want["state"][:4].tolist(), got["state"].tolist()
    for k in ("beam_scores", "hyp_score", "worst"):
        err, w = np.abs(got[k].astype(np.float64) - want[k]).ravel(), np.ravel(want[k + "_w"])
        assert (err <= w).all(), ("beam", k, float(err.max()))
    print(f"select-dist | beam | exact: {got['tokens'].size} tokens, sources, histories and candidate counts are select_ref's")
    judge(S.beam_checks(got["tokens"]) + S.beam_controls(got["tokens"]))
