"""itts_sample_rows through the C ABI: the token-selection step with one 32-byte record of sampling settings per row.

Every row is held to oracle/sampling_ref.py applied to that row ALONE under its own record (process -> uniform01(seed, stream,
row step) -> pick | greedy); the launch as a whole to itts_sample where the two must coincide (equal records, stream = row)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
STOP = 8193
B = 6
CAP = 16
# One record per row; between them every field differs: greedy | top_k 1, 30, 1024 | top_p 0.3, 0.8, 1.0 | temperature 0.7, 1.3 |
# penalty 1.0, 10.0 | seeds above 2^32 | streams that are not the row index.  Row 5's logits make its top-p set a single token.
RECORDS = [
    dict(do_sample=False, temperature=1.0, top_k=1, top_p=1.0, repetition_penalty=10.0, seed=(1 << 33) + 1, stream=7),
    dict(do_sample=True, temperature=0.7, top_k=1, top_p=1.0, repetition_penalty=1.0, seed=(1 << 32) + 5, stream=3),
    dict(do_sample=True, temperature=1.3, top_k=30, top_p=0.8, repetition_penalty=10.0, seed=(1 << 40) + 9, stream=0),
    dict(do_sample=True, temperature=0.7, top_k=1024, top_p=0.3, repetition_penalty=10.0, seed=(1 << 63) + 2, stream=11),
    dict(do_sample=True, temperature=1.3, top_k=1024, top_p=1.0, repetition_penalty=1.0, seed=(3 << 32), stream=(1 << 32) - 1),
    dict(do_sample=True, temperature=0.7, top_k=30, top_p=0.3, repetition_penalty=10.0, seed=(1 << 32) + 77, stream=2),
]


@pytest.fixture(scope="module")
def nat():
    from indextts import _native
    return _native


def make_inputs(V, seed):
    """fp32 logits [B, V], a history [B, CAP] and the always-penalised ids.  Exact ties: row 0's two best scores, the 30th / 31st
    best of rows 2 and 5 (both are kept by top-k 30), two mid-rank scores of row 3.  Row 5: one token far above the rest."""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((B, V)) * 3.0).astype(np.float32)
    order = np.argsort(-lg, axis=1, kind="stable")
    lg[0, order[0, 1]] = lg[0, order[0, 0]]
    lg[2, order[2, 30]] = lg[2, order[2, 29]]
    lg[5, order[5, 30]] = lg[5, order[5, 29]]
    lg[3, order[3, 500]] = lg[3, order[3, 499]]
    lg[5, order[5, 0]] += np.float32(40.0)
    hist = rng.integers(0, V, size=(B, CAP)).astype(np.int32)
    hist[:, 1] = order[:, 0]           # the best token is in every row's history from step 2 on: the penalty changes the winner
    hist[2, 2] = hist[2, 0]            # a repeated id is penalised once
    extra = np.array([1, V - 2], dtype=np.int32)
    return lg, hist, extra


def expected(lg_row, ids, rec, k_b):
    """(processed scores, token) of one row alone under its record, from the oracle."""
    from oracle import sampling_ref as ref
    if rec["do_sample"]:
        sc = ref.process(lg_row[None], ids[None], rec["repetition_penalty"], rec["temperature"], rec["top_k"], rec["top_p"])[0]
        return sc, ref.pick(sc, ref.uniform01(rec["seed"], rec["stream"], k_b))
    sc = ref.process(lg_row[None], ids[None], rec["repetition_penalty"], 1.0, 0, None)[0]
    return sc, int(ref.greedy(sc[None])[0])


def top_p_margin(lg_row, ids, rec):
    """Distance of the oracle's ascending cumulative probabilities from the top-p cut 1 - p: a cut closer than fp32 summation
    order can move (~1e-6) would make the kept set a matter of rounding, in the oracle as much as in the kernel."""
    from oracle import sampling_ref as ref
    sc = ref.process(lg_row[None], ids[None], rec["repetition_penalty"], rec["temperature"], rec["top_k"], None)[0]
    s = np.sort(sc[np.isfinite(sc)])
    cum = np.cumsum(ref._softmax(s[None])[0], dtype=np.float32)
    return float(np.abs(cum - np.float32(1.0 - rec["top_p"])).min())


def launch(nat, lg, hist, extra, rows, step, row_step0=None, force=None, finished=None, dbg=True, no_advance=False):
    """One itts_sample_rows launch at loop step `step`; returns host copies of what it wrote."""
    Bn, V = lg.shape
    t = dict(tokens=torch.full((Bn,), -5, dtype=torch.int32, device=DEV),
             history=torch.from_numpy(hist).to(DEV).contiguous(),
             finished=torch.zeros(Bn, dtype=torch.int32, device=DEV) if finished is None else torch.tensor(finished, dtype=torch.int32, device=DEV),
             state=torch.zeros(8, dtype=torch.int32, device=DEV))
    t["state"][0] = step
    t["state"][1] = 100 + step
    d = torch.empty(Bn, V, dtype=torch.float32, device=DEV) if dbg else None
    nat.sample_rows(torch.from_numpy(lg).to(DEV), t["tokens"], t["history"], t["finished"], t["state"], torch.from_numpy(extra).to(DEV),
                    None if force is None else torch.tensor(force, dtype=torch.int32, device=DEV), rows, STOP, d, no_advance=no_advance,
                    row_step0=None if row_step0 is None else torch.tensor(row_step0, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["dbg"] = None if d is None else d.cpu().numpy()
    return out


def check_row(got, b, sc, tok, what):
    d = got["dbg"][b]
    assert np.array_equal(np.isfinite(d), np.isfinite(sc)), (what, "kept set", int(np.isfinite(d).sum()), int(np.isfinite(sc).sum()))
    np.testing.assert_allclose(d[np.isfinite(d)], sc[np.isfinite(sc)], rtol=1e-6)   # the bound of test_sample_matches_hf_fixture
    assert int(got["tokens"][b]) == tok, (what, int(got["tokens"][b]), tok)


@pytest.mark.parametrize("V", [8194, 1000])
def test_every_row_follows_the_oracle_under_its_own_record(nat, V):
    """B = 6 rows whose records differ in every field, steps 0..3 with a history and extra ids, V = 8194 (the real vocabulary:
    what the candidate store is sized for) and V = 1000 (top_k 1024 exceeds it).  Per row: the processed scores have the oracle's
    finite set and values (rtol 1e-6, as the scalar form's fixture test), the token is the oracle's."""
    lg, hist, extra = make_inputs(V, 100 + V)
    kept_single = False
    for step in range(4):
        got = launch(nat, lg, hist, extra, RECORDS, step)
        assert got["state"][0] == step + 1 and got["state"][1] == 101 + step and got["state"][3] == 0
        for b, rec in enumerate(RECORDS):
            ids = np.concatenate([extra, hist[b, :step]])
            if rec["do_sample"] and rec["top_p"] < 1.0:
                assert top_p_margin(lg[b], ids, rec) > 1e-5, ("test data: a top-p cut on a rounding edge", V, step, b)
            sc, tok = expected(lg[b], ids, rec, step)
            check_row(got, b, sc, tok, (V, step, b))
            assert got["history"][b, step] == tok and np.array_equal(got["history"][b, :step], hist[b, :step])
            kept_single |= b == 5 and int(np.isfinite(sc).sum()) == 1
        assert int(np.isfinite(got["dbg"][2]).sum()) >= 2          # (row 2 keeps several candidates: its draw is a real draw)
    assert kept_single, "row 5 was built to keep a single token under top-p"


@pytest.mark.parametrize("do_sample", [True, False])
def test_equal_records_with_stream_b_are_the_scalar_form_bit_for_bit(nat, do_sample):
    """Every record the same and stream = row index: tokens, history, finished flags, loop state and processed scores equal an
    itts_sample launch with those scalars -- including a row stopped by force_stop and one that had finished before."""
    V, step, seed = 8194, 3, (1 << 35) + 12345
    lg, hist, extra = make_inputs(V, 7)
    lg[1, STOP] = 900.0                                             # row 1 draws / takes the stop token itself
    rec = dict(do_sample=do_sample, temperature=0.7, top_k=30, top_p=0.8, repetition_penalty=10.0, seed=seed)
    force, fin = [-1, -1, 3, -1, -1, -1], [0, 0, 0, 0, 1, 0]
    for no_advance in (False, True):
        got = launch(nat, lg, hist, extra, [dict(rec, stream=b) for b in range(B)], step, force=force, finished=fin, no_advance=no_advance)
        t = dict(tokens=torch.full((B,), -5, dtype=torch.int32, device=DEV), history=torch.from_numpy(hist).to(DEV).contiguous(),
                 finished=torch.tensor(fin, dtype=torch.int32, device=DEV), state=torch.zeros(8, dtype=torch.int32, device=DEV))
        t["state"][0], t["state"][1] = step, 100 + step
        dbg = torch.empty(B, V, dtype=torch.float32, device=DEV)
        nat.sample(torch.from_numpy(lg).to(DEV), t["tokens"], t["history"], t["finished"], t["state"], torch.from_numpy(extra).to(DEV),
                   torch.tensor(force, dtype=torch.int32, device=DEV), 10.0, 0.7, 30, 0.8, do_sample, seed, STOP, dbg, no_advance=no_advance)
        torch.cuda.synchronize()
        for k, v in t.items():
            assert np.array_equal(got[k], v.cpu().numpy()), (k, no_advance)
        assert np.array_equal(got["dbg"].view(np.uint32), dbg.cpu().numpy().view(np.uint32))
        assert got["tokens"][1] == STOP and got["tokens"][2] == STOP and got["tokens"][4] == STOP
        assert got["finished"].tolist() == [0, 1, 1, 0, 1, 0] and got["state"][2] == 2
        assert got["state"][0] == (step if no_advance else step + 1)


def test_a_row_counts_its_own_steps(nat):
    """row_step0 = [2, 5] at loop step 5: row 0 is at its step 3 (draws uniform01(seed, stream, 3), penalises history[0][:3], appends
    at index 3), row 1 at its step 0 (no history of its own yet) -- whatever the loop's step."""
    V = 8194
    lg, hist, extra = make_inputs(V, 11)
    lg, hist = lg[[2, 5]], hist[[2, 5]]
    recs = [RECORDS[2], dict(RECORDS[4], repetition_penalty=10.0)]
    got = launch(nat, lg, hist, extra, recs, 5, row_step0=[2, 5])
    for b, k_b in enumerate((3, 0)):
        sc, tok = expected(lg[b], np.concatenate([extra, hist[b, :k_b]]), recs[b], k_b)
        check_row(got, b, sc, tok, ("own clock", b))
        assert got["history"][b, k_b] == tok
        keep = np.ones(CAP, dtype=bool)
        keep[k_b] = False
        assert np.array_equal(got["history"][b][keep], hist[b][keep])
    # the loop's step would have given other numbers: the row's own step is what addresses the draw
    from oracle import sampling_ref as ref
    assert ref.uniform01(recs[0]["seed"], recs[0]["stream"], 3) != ref.uniform01(recs[0]["seed"], recs[0]["stream"], 5)


def test_rows_are_independent(nat):
    """Permuting the rows of logits, history and table permutes the tokens (stream and seed travel in the record)."""
    V = 8194
    lg, hist, extra = make_inputs(V, 13)
    perm = [4, 2, 5, 0, 3, 1]
    a = launch(nat, lg, hist, extra, RECORDS, 2, dbg=False)
    b = launch(nat, lg[perm], hist[perm], extra, [RECORDS[i] for i in perm], 2, dbg=False)
    assert np.array_equal(b["tokens"], a["tokens"][perm]) and np.array_equal(b["history"], a["history"][perm])
    assert len(set(a["tokens"].tolist())) > 1


def test_records_nobody_checked_are_clamped(nat):
    """Records written straight into the device table, past the wrapper's checks: top_k = 0 and 5000, temperature = 0, penalty = 0.
    The launch returns normally with tokens inside [0, V) -- the tokens of the clamped settings: top_k 1 and min(V, 1024),
    temperature 1, penalty 1.  (A check of the clamp, not of faults: nothing here may index out of range.)"""
    for V in (8194, 1000):
        lg, hist, extra = make_inputs(V, 17)
        base = dict(do_sample=True, temperature=0.7, top_k=30, top_p=0.8, repetition_penalty=10.0, seed=(1 << 34) + 3)
        raw = [dict(base, top_k=0), dict(base, top_k=5000), dict(base, temperature=0.0), dict(base, repetition_penalty=0.0),
               dict(base, top_k=-7, top_p=1.0), dict(base, do_sample=False, top_k=0, temperature=0.0)]
        ok = [dict(base, top_k=1), dict(base, top_k=1024), dict(base, temperature=1.0), dict(base, repetition_penalty=1.0),
              dict(base, top_k=1, top_p=1.0), dict(base, do_sample=False)]
        recs = (nat.SampleRow * B)()
        for b, (rec, d) in enumerate(zip(recs, raw)):
            rec.rep_penalty, rec.temperature, rec.top_p, rec.top_k = d["repetition_penalty"], d["temperature"], d["top_p"], d["top_k"]
            rec.seed, rec.stream, rec.do_sample = d["seed"], b + 1, int(d["do_sample"])
        assert ctypes.sizeof(recs) == B * 32
        table = torch.from_numpy(np.frombuffer(bytes(recs), dtype=np.uint8).reshape(B, 32).copy()).to(DEV)
        got = launch(nat, lg, hist, extra, table, 3)
        want = launch(nat, lg, hist, extra, [dict(d, stream=b + 1) for b, d in enumerate(ok)], 3)
        assert ((got["tokens"] >= 0) & (got["tokens"] < V)).all(), got["tokens"]
        assert np.array_equal(got["tokens"], want["tokens"])
        assert np.array_equal(got["dbg"].view(np.uint32), want["dbg"].view(np.uint32))


def test_wrapper_refuses_before_launching(nat):
    lg, hist, extra = make_inputs(1000, 19)
    for bad in (dict(top_k=0), dict(top_k=1025), dict(top_p=0.0), dict(temperature=0.0), dict(repetition_penalty=0.0)):
        with pytest.raises(ValueError):
            launch(nat, lg, hist, extra, RECORDS[:5] + [dict(RECORDS[5], **bad)], 0)
    with pytest.raises(ValueError):
        launch(nat, lg, hist, extra, RECORDS[:5], 0)
    with pytest.raises(nat.NativeError):                                # a table for fewer rows than the logits have
        launch(nat, lg, hist, extra, torch.zeros(B - 1, 32, dtype=torch.uint8, device=DEV), 0)
