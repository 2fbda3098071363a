"""The token-selection kernels through the C ABI against tests/select_ref.py, one launch per case from the state the case uploads
(nothing compounds: a failure names its case, and the case names its arms): itts_sample and itts_sample_rows (csrc/sampling.hip),
itts_beam_step and itts_beam_kv_rows (csrc/beam.hip).  What the reference computes exactly is compared with ==; what sits behind an
expf / logf is compared within the budget select_ref derives, on data whose decisions clear that budget
(tests/test_select_ref_cpu.py).  Every check prints one `select | arms | case | margin / budget` line (profiles/select_kernels.txt)."""
import numpy as np
import pytest
import torch

from tests import select_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMPLER = R.sampler_cases()
BEAM = R.beam_cases()
KV = R.kv_cases()


@pytest.fixture(scope="module")
def nat():
    from indextts import _native
    return _native


def note(arms, what, value):
    print(f"select | {' '.join(sorted(arms))} | {what} | {value:.3g}")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def padded(lg, pad):
    """The logits with `pad` columns of 1e30 behind every row: a [rows, V] view of row stride V + pad."""
    buf = np.full((lg.shape[0], lg.shape[1] + pad), 1e30, dtype=np.float32)
    buf[:, : lg.shape[1]] = lg
    return dev(buf)[:, : lg.shape[1]]


def state_words(c, step, pos):
    st = np.zeros(8, dtype=np.uint32)
    st[0], st[1], st[4], st[5] = step, pos, c["s45"][0], c["s45"][1]
    return dev(st.view(np.int32))


def launch_sampler(nat, c, no_advance, rows):
    B, V = c["lg"].shape
    t = dict(tokens=torch.full((B,), -5, dtype=torch.int32, device=DEV), history=dev(c["hist"]), finished=dev(np.array(c["finished"], dtype=np.int32)),
             state=state_words(c, c["step"], c["pos"]), dbg=torch.full((B, V), 7.0, dtype=torch.float32, device=DEV))
    extra = dev(c["extra"]) if c["extra"].shape[0] else None
    force = None if c["force"] is None else dev(np.array(c["force"], dtype=np.int32))
    lg = padded(c["lg"], c["pad"])
    if rows:
        recs = [dict(do_sample=c["do_sample"], temperature=c["temp"], top_k=c["top_k"], top_p=c["top_p"], repetition_penalty=c["rep"],
                     seed=c["seed"], stream=b) for b in range(B)]
        nat.sample_rows(lg, t["tokens"], t["history"], t["finished"], t["state"], extra, force, recs, c["stop"], t["dbg"], no_advance=no_advance)
    else:
        nat.sample(lg, t["tokens"], t["history"], t["finished"], t["state"], extra, force, c["rep"], c["temp"], c["top_k"], c["top_p"],
                   c["do_sample"], c["seed"], c["stop"], t["dbg"], no_advance=no_advance)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def check_sampler(c, want, got, what):
    B, V = c["lg"].shape
    cap = c["hist"].shape[1]
    for b, r in enumerate(want["rows"]):
        d = got["dbg"][b]
        if r["overflow"]:
            # more than 1024 scores at the k-th value: WHICH 1024 stay is the LDS atomicAdd's order -- only membership is specified
            fin = np.nonzero(np.isfinite(d))[0]
            assert fin.shape[0] == R.MAXC and np.isin(fin, r["kept"]).all(), (what, b, fin.shape[0])
            assert np.array_equal(d[fin].view(np.uint32), r["scores"][fin].view(np.uint32)) and np.all(d[~np.isfinite(d)] == -np.inf), (what, b)
            tok = int(got["tokens"][b])
            assert tok in fin, (what, b, tok)
            if c["step"] < cap:
                assert got["history"][b, c["step"]] == tok
                want["history"][b, c["step"]] = tok
            want["tokens"][b] = tok
            continue
        assert np.array_equal(np.isfinite(d), np.isfinite(r["dbg"])), (what, b, "kept set", int(np.isfinite(d).sum()), int(np.isfinite(r["dbg"]).sum()))
        assert np.array_equal(d.view(np.uint32), r["dbg"].view(np.uint32)), (what, b, "processed scores: bits")
    assert got["tokens"].tolist() == want["tokens"], (what, got["tokens"].tolist(), want["tokens"])
    assert np.array_equal(got["history"], want["history"]), (what, "history")
    assert np.array_equal(got["finished"], want["finished"]), (what, "finished")
    assert got["state"][:4].tolist() == want["state"][:4].tolist(), (what, got["state"].tolist(), want["state"].tolist())


@pytest.mark.parametrize("c", SAMPLER, ids=[c["name"] for c in SAMPLER])
def test_sampler_case(nat, c):
    """itts_sample under both no_advance values against the reference (processed scores bit for bit, token, history row, finished
    flags, state[0..3]), and itts_sample_rows with equal records and stream = row bit-equal to itts_sample.  The `overflow` case
    (all logits equal: 8194 scores tied at the k-th value) only requires the token to lie in the reference's kept set and the
    1024 survivors to be members with the right scores: two launches need NOT agree on which 1024 stay, so the two forms are
    not compared with each other there."""
    for no_advance in (False, True):
        want = R.sample_case(c, no_advance)
        assert want["arms"] == c["arms"] and want["margin"] > 1.0
        got = launch_sampler(nat, c, no_advance, rows=False)
        check_sampler(c, want, got, (c["name"], "itts_sample", no_advance))
        got2 = launch_sampler(nat, c, no_advance, rows=True)
        if any(r["overflow"] for r in want["rows"]):
            check_sampler(c, R.sample_case(c, no_advance), got2, (c["name"], "itts_sample_rows", no_advance))
        else:
            for k in got:
                assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                      got2[k].view(np.uint32) if got2[k].dtype == np.float32 else got2[k]), (c["name"], "rows form", k, no_advance)
    note(c["arms"], c["name"], want["margin"])


def launch_beam(nat, c):
    R_, V = c["lg"].shape
    B, nb = c["B"], c["nb"]
    i32 = dict(dtype=torch.int32, device=DEV)
    t = dict(tokens=torch.full((R_,), -5, **i32), src=torch.full((R_,), -5, **i32), beam_scores=dev(c["beam_scores"]), hist=dev(c["hist"]),
             hyp_score=dev(c["hyp_score"]), hyp_len=dev(c["hyp_len"]), hyp_tok=dev(c["hyp_tok"]), n_hyp=dev(c["n_hyp"]), worst=dev(c["worst"]),
             done=dev(c["done"]), state=state_words(c, c["step"], c["pos"]))
    scratch = (torch.full((R_, 1024), 3.0, device=DEV), torch.full((R_, 1024), -1, **i32), torch.full((R_,), -1, **i32))
    nat.beam_step(padded(c["lg"], c["pad"]), nb, t["tokens"], t["src"], t["beam_scores"], t["hist"], t["hyp_score"], t["hyp_len"], t["hyp_tok"],
                  t["n_hyp"], t["worst"], t["done"], t["state"], dev(c["extra"]) if c["extra"].shape[0] else None, c["rep"], c["temp"], c["top_k"],
                  c["top_p"], c["do_sample"], c["lp"], c["seed"], c["eos"], scratch=scratch)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["cand_n"] = scratch[2].cpu().numpy()
    return out


def within(got, want, w):
    """Worst |got - want| / budget; a budget of 0 (an exact value) asks for equality."""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(w > 0, err / w, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


@pytest.mark.parametrize("c", BEAM, ids=[c["name"] for c in BEAM])
def test_beam_case(nat, c):
    """One itts_beam_step launch: tokens, source rows, done flags, hypothesis counts / lengths / tokens, both history planes, the loop
    state and every row's candidate count with ==; beam_scores, hyp_score and worst within the derived score budget."""
    want = R.beam_case(c)
    assert want["arms"] == c["arms"] and want["margin"] > 1.0
    got = launch_beam(nat, c)
    assert got["cand_n"].tolist() == want["cand_n"].tolist(), (c["name"], "cand_n", got["cand_n"].tolist(), want["cand_n"].tolist())
    for k in ("tokens", "src", "done", "n_hyp", "hyp_len", "hyp_tok", "hist"):
        assert np.array_equal(got[k], want[k].reshape(got[k].shape)), (c["name"], k, got[k].tolist() if got[k].size < 64 else "", want[k].tolist() if got[k].size < 64 else "")
    assert got["state"][:4].tolist() == want["state"][:4].tolist(), (c["name"], got["state"].tolist())
    worst = 0.0
    for k in ("beam_scores", "hyp_score", "worst"):
        r = within(got[k], want[k], want[k + "_w"])
        assert r <= 1.0, (c["name"], k, r, got[k].tolist(), want[k].tolist())
        worst = max(worst, r)
    note(c["arms"], c["name"], want["margin"])
    note({"scores"}, c["name"] + ": err / budget of beam_scores, hyp_score, worst", worst)


@pytest.mark.parametrize("c", KV, ids=[c["name"] for c in KV])
def test_beam_kv_rows_case(nat, c):
    """itts_beam_kv_rows: the whole table (both parities) equals the rule's, entry for entry."""
    tbl, st = dev(c["tbl"]), np.zeros(8, dtype=np.int32)
    st[0], st[1] = c["k1"], c["P"]
    nat.beam_kv_rows(tbl, dev(c["src"]), dev(st))
    torch.cuda.synchronize()
    assert np.array_equal(tbl.cpu().numpy(), R.kv_rows_ref(c["tbl"], c["src"], c["k1"], c["P"])), c["name"]
    note({"kv-rows"}, c["name"], float("inf"))
