"""Reference, case table, arm predictor and decision margins for the token-selection kernels (csrc/sampling.hip: itts_sample,
itts_sample_rows; csrc/beam.hip: itts_beam_step, itts_beam_kv_rows).  Host only (numpy); imports neither the native library nor
oracle/ -- tests/test_select_ref_cpu.py holds it to the oracles, tests/test_select_kernels_gpu.py holds the kernels to it.

TWO LAYERS, split where the kernels round.

Exact layer (sampler).  The repetition penalty is one IEEE fp32 multiply or divide, the temperature one fp32 divide, and the library
is built without a fast-math flag (csrc/Makefile), so doing both in np.float32 gives the kernel's bits.  Top-k membership (ties with
the k-th value kept), the greedy token (lowest id on ties) and the (score descending, id ascending) order are comparisons of those
bits: the tests compare them with == on the uint32 view, no tolerance.

Rounded layer.  Everything behind an expf / logf is computed here in float64 from the exact fp32 scores, and every DECISION the
kernel takes on such a quantity carries a margin: the distance of the float64 quantity from the decision's edge, which has to exceed
the budget below.  A case whose margin does not exceed its budget is bad test data (tests/test_select_ref_cpu.py refuses it);
the budget is never fitted to a device.  eps = 2^-24 is the unit roundoff of fp32 (round to nearest), so one rounded operation
has relative error <= eps and one ulp is <= 2 eps relative.

  ASSUMPTION: the device expf and logf are within U = 3 ulp, powf within 16 ulp.  The ROCm device-library documentation is not
  shipped with the toolchain this was written against (only its licence file is), so the figures are the OpenCL full-profile
  bounds, which the device library is built to meet (its own table claims 1 ulp for exp and log).

  numerators  c_i = expf(s_i - s_0): the fp32 subtraction is off by <= eps |d_i| (d_i = s_i - s_0), which expf turns into a relative
      error eps |d_i|, plus U ulp of expf itself:  |delta_i| <= eps |d_i| + 2 U eps.  E(S) = sum_{i in S} c_i |delta_i| / sum_S c_i
      is the numerators' share in any sum over S, relative to that sum.  expf(-inf) = 0 and expf(0) = 1 are exact.
  total       n - 1 fp32 additions in the kernel's order (descending index): relative error <= (n - 1) eps + E.
  top-p       cum_i = sum_{j >= i} fl(c_j / total), m = n - i terms: one division (eps) and one addition (eps) per term, the
      total's error on every term:  |cum_fl - cum| <= cum (n + m + 1) eps + 2 E.  The edge 1 - top_p is an fp32 subtraction of fp32
      values: done here in np.float32, exact layer.  Decision: cum_i <= 1 - top_p, for every i the loop reaches.
  draw        tot2 = sum_{i < keep} c_i (keep - 1 additions), dthr = fl(u tot2) (one multiply), run_j = j additions.  Relative
      to tot2:  |run_fl - run| / tot2 <= (run / tot2)(j + 1) eps + E2 and |dthr_fl - u tot2| / tot2 <= u (keep + 1) eps + E2 with
      E2 = E(kept).  Decision: run_j > u tot2 for every j up to the pick.  u = (x >> 8) 2^-24 is exact.
  all-tied    when every kept score equals s_0 and n is a power of two every quantity above is a dyadic rational the fp32 chain
      represents exactly (c_i = 1, total = n, 1 / n, their sums): budget 0, a decision ON the edge is then specified too
      (cum == 1 - top_p is removed).

Beam (phase 1, per row).  The scores are log-probabilities, so even the top-k runs on rounded values:
      se = sum expf(l_i - max): per-thread partial sums (33 additions), a 6-level wave tree, a 2-level block tree: <= 41 eps, plus
      the numerators' E;  lse = max + logf(se): U ulp of logf on |log se| and one addition:
          A = 41 eps + E + 2 U eps |log se| + eps |lse|
      v = l - lse: A + eps |v|;  penalty (v rep or v / rep): the error times rep (or 1 / rep) + eps |v'|;  temperature: the error
      / t + eps |v''|.  That is w_i, the score budget of candidate i.  Two candidates with the same logit bits and the same penalty
      flag go through the same operations: their tie is exact.  Any other pair the kernel orders (the k-th value against the next
      one below, neighbours in the sorted candidate list) needs a gap > w_a + w_b.  Top-p numerators expf(s_i - s_0) carry w_i + w_0
      on top of the sampler's delta_i.
Beam (phase 2).  P = fl(s + beam_score).  If rounding s - w and s + w to fp32 and adding the beam score gives the same fp32 value,
      P is that value, exactly (this is what happens at step 0: -1e9 + v is -1e9 for every |v| < 32); otherwise its budget is
      w + eps |P|.  Pool order: neighbours in the sorted pool need a gap > the sum of their budgets, or an exact tie (then the flat
      index decides).  Draws: as the sampler's, over np pool entries (dead entries add +0).  Hypothesis score hs = P / gen^lp: the
      budget of P divided by gen^lp, + eps |hs|, + 16 ulp of powf when length_penalty != 0; `hs > worst`, the eviction's argmin and
      `worst >= best / gen^lp` are decisions with that budget.  beam_scores, hyp_score and worst are COMPARED within these budgets.

CAPACITY RULES (include/indextts_hip.h says the same): the beam pool is the beams' sorted candidate lists concatenated in beam
order and cut at 1024 entries BEFORE it is sorted.  A sampler row with more than 1024 scores at or above the k-th value keeps
whichever 1024 win the kernel's LDS atomicAdd: the reference returns the whole kept set and flags the row `overflow`; only the
token's membership in that set is specified, two launches need not agree.

Philox4x32-10 is restated here (python integers) with the two counters -- sampler (row | stream, step, 0, 0), beam
(b, step, draw, 0) -- and the key seed + state[4..5] with the 64-bit carry.

`MUTANTS` are the reference with one rule wrong each (the `rules` argument of the reference functions); the CPU test shows that
each of them changes something the GPU test compares, on at least one case of the table."""
import math

import numpy as np

EPS = 2.0 ** -24
U_EXP = U_LOG = 3.0
U_POW = 16.0
MAXC = 1024          # candidate store of a sampler row, of a beam row, and the beam pool
M32 = 0xFFFFFFFF
F32, F64 = np.float32, np.float64
INF = math.inf

MUTANTS = ("kth-tie-dropped", "top-p-strict", "beam-min-keep-1", "dup-penalised-twice", "out-of-range-wrapped", "tie-break-reversed",
           "philox-words-swapped", "seed-carry-dropped", "pool-cut-after-sort", "eos-rank-off-by-one")

SAMPLER_ARMS = ("fast", "fast-trim", "overflow-bisect", "bisect", "overflow", "tail<=64", "tail>64", "top_p<1", "top_p=1", "keep=1",
                "greedy", "penalty-dup", "penalty-out-of-range", "penalty-zero", "hist-capped", "forced")
BEAM_ARMS = ("b:fast", "b:fast-trim", "b:overflow-bisect", "b:top_p<1", "b:top_p=1", "b:min-keep-2", "b:search", "b:penalty-dup",
             "b:penalty-out-of-range", "b:hist-capped", "b:step0", "pool-cut", "draw-fallback", "eos-closes", "eos-low-rank-dropped",
             "evict-worst", "eos-worse", "fill-from-first-beam", "done-row", "becomes-done")
ARMS = SAMPLER_ARMS + BEAM_ARMS


# ------------------------------------------------------------------------------------------------------------------ Philox
def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_key(seed, s4, s5, rules=()):
    """Launch argument `seed` (64 bits) + the 64-bit value held in state[4] (low word) and state[5] (high word)."""
    seed, s4, s5 = int(seed) & (2 ** 64 - 1), int(s4) & M32, int(s5) & M32
    if "seed-carry-dropped" in rules:
        return ((seed & M32) + s4) & M32, ((seed >> 32) + s5) & M32
    k = (seed + ((s5 << 32) | s4)) & (2 ** 64 - 1)
    return k & M32, k >> 32


def uniform(ctr, key, rules=()):
    if "philox-words-swapped" in rules:
        ctr = (ctr[1], ctr[0]) + tuple(ctr[2:])
    return F32(philox4x32_10(ctr, key)[0] >> 8) * F32(2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------ shared
def fkey(x):
    """The kernels' order-preserving uint32 key of an fp32 value."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def route(scores32, kk):
    """Host mirror of the top-k threshold's branch: thread t of 256 owns ids t + 256 i; the fast bound is the kk-th largest of the
    256 per-thread maxima."""
    if kk > 256:
        return {"bisect"}
    keys = np.zeros(-(-scores32.shape[0] // 256) * 256, dtype=np.uint32)
    keys[: scores32.shape[0]] = fkey(scores32)
    bound = np.sort(keys.reshape(-1, 256).max(0))[::-1][kk - 1]
    cnt = int((keys >= bound).sum())
    if cnt > MAXC:
        return {"overflow-bisect"}
    return {"fast", "fast-trim"} if cnt > kk else {"fast"}


def penalty_ids(ids, V, rules=()):
    """(ids the penalty is applied to -- with repeats only under the mutant --, arms)."""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < V)
    arms = set()
    if not ok.all():
        arms.add("penalty-out-of-range")
    ids = ids % V if "out-of-range-wrapped" in rules else ids[ok]
    if np.unique(ids).shape[0] < ids.shape[0]:
        arms.add("penalty-dup")
    return (ids if "dup-penalised-twice" in rules else np.unique(ids)), arms


def ratio(margin, budget):
    return INF if budget == 0.0 else margin / budget


def sort_order(scores, ids, rules=()):
    return np.lexsort((-ids if "tie-break-reversed" in rules else ids, -scores))


def tail(s_sorted, w_sorted, top_p, u, min_keep, rules=(), draw=True):
    """The part both kernels share behind the sorted candidate list: numerators, top-p cut, inverse-CDF draw.  s_sorted float64
    (descending), w_sorted their score budgets (zeros: exact).  Returns (keep, pick index or None, worst margin / budget)."""
    n = s_sorted.shape[0]
    d = s_sorted - s_sorted[0]
    e = np.exp(d)
    exact = bool(np.all(d == 0) and np.all(w_sorted == 0) and n & (n - 1) == 0)
    with np.errstate(invalid="ignore"):
        delta = np.where(e > 0, np.where(d == 0, 0.0, np.abs(d) * EPS + 2 * U_EXP * EPS) + w_sorted + w_sorted[0], 0.0)
    if exact:
        delta[:] = 0.0
    total = e.sum()
    E = float((e * delta).sum() / total)
    worst = INF
    keep = n
    if top_p < 1.0 and n > min_keep:
        lim = F64(F32(1.0) - F32(top_p))
        cum = np.cumsum(e[::-1])[: n - min_keep] / total            # cum[m - 1]: the m lowest candidates, i = n - m
        rem = cum < lim if "top-p-strict" in rules else cum <= lim
        stop = int(np.argmin(rem)) if not rem.all() else rem.shape[0]   # first decision that says "stays"
        keep = n - stop
        seen = min(stop + 1, rem.shape[0])                             # the decisions the loop takes
        m = np.arange(1, seen + 1)
        budget = 0.0 if exact else cum[:seen] * (n + m + 1) * EPS + 2 * E
        mg = np.abs(cum[:seen] - lim)
        worst = INF if exact else float(np.min(mg / budget))
    if not draw:
        return keep, None, worst
    ek = e[:keep]
    tot2 = ek.sum()
    E2 = float((ek * delta[:keep]).sum() / tot2)
    run = np.cumsum(ek) / tot2
    hit = np.nonzero(run > F64(u))[0]
    pick = int(hit[0]) if hit.shape[0] else keep - 1
    if keep > 1 and not exact:
        j = np.arange(0, min(pick + 1, keep - 1))                        # (the last kept candidate is taken either way)
        budget = run[j] * (j + 1) * EPS + F64(u) * (keep + 1) * EPS + 2 * E2
        worst = min(worst, float(np.min(np.abs(run[j] - F64(u)) / budget)))
    return keep, pick, worst


# ------------------------------------------------------------------------------------------------------------------ sampler
def sample_row(lg, ids, rep, temp, top_k, top_p, do_sample, u, rules=()):
    """One row of itts_sample.  lg fp32 [V]; ids = extra ids + the row's history window.  Returns a dict: `scores` (fp32 [V], exact
    layer), `dbg` (what dbg_scores holds), `kept` (ids, sorted), `n`, `keep`, `token` (None when `overflow`), `arms`, `margin`."""
    V = lg.shape[0]
    s = lg.astype(F32).copy()
    arms = set()
    if F32(rep) != F32(1.0):
        pid, arms = penalty_ids(ids, V, rules)
        if pid.shape[0] and np.any(s[pid] == 0):
            arms.add("penalty-zero")
        for chunk in ([pid] if "dup-penalised-twice" not in rules else [pid[i:i + 1] for i in range(pid.shape[0])]):
            with np.errstate(invalid="ignore", over="ignore"):
                s[chunk] = np.where(s[chunk] < 0, s[chunk] * F32(rep), s[chunk] / F32(rep))
    allid = np.arange(V)
    if not do_sample:
        best = allid[s == s.max()]
        tok = int(best.max() if "tie-break-reversed" in rules else best.min())
        return dict(scores=s, dbg=s.copy(), kept=np.array([tok]), n=1, keep=1, token=tok, overflow=False, arms=arms | {"greedy"}, margin=INF)
    if F32(temp) != F32(1.0):
        s = (s / F32(temp)).astype(F32)
    kk = min(int(top_k), V, MAXC)
    order = sort_order(s, allid, rules)
    kth = s[order[kk - 1]]
    n = kk if "kth-tie-dropped" in rules else int((s >= kth).sum())
    arms |= route(s, kk)
    dbg = np.full(V, -np.inf, dtype=F32)
    if n > MAXC:
        kept = order[:n]
        dbg[kept] = s[kept]
        return dict(scores=s, dbg=dbg, kept=kept, n=n, keep=None, token=None, overflow=True, arms=arms | {"overflow"}, margin=INF)
    kept = order[:n]
    keep, pick, worst = tail(s[kept].astype(F64), np.zeros(n), float(F32(top_p)), u, 1, rules)
    arms |= {"tail<=64" if n <= 64 else "tail>64", "top_p<1" if F32(top_p) < F32(1.0) else "top_p=1"}
    if keep == 1:
        arms.add("keep=1")
    dbg[kept[:keep]] = s[kept[:keep]]
    return dict(scores=s, dbg=dbg, kept=kept[:keep], n=n, keep=keep, token=int(kept[pick]), overflow=False, arms=arms, margin=worst)


def sample_case(c, no_advance=False, rules=()):
    """One launch of itts_sample from the state the case uploads.  Returns the expected outputs: tokens (None: overflow row),
    history, finished, state (int64 [8]; words 4..5 as uploaded), dbg [B, V], rows (the per-row dicts), arms, margin."""
    lg, hist = c["lg"], c["hist"]
    B, V = lg.shape
    cap = hist.shape[1]
    step = c["step"]
    key = philox_key(c["seed"], c["s45"][0], c["s45"][1], rules)
    out_hist, fin = hist.copy(), np.array(c["finished"], dtype=np.int32)
    state = np.array([step, c["pos"], 0, 0, c["s45"][0], c["s45"][1], 0, 0], dtype=np.int64)
    tokens, rows, arms, worst = [], [], set(), INF
    for b in range(B):
        ids = np.concatenate([c["extra"], hist[b, : min(step, cap)]])
        r = sample_row(lg[b], ids, c["rep"], c["temp"], c["top_k"], c["top_p"], c["do_sample"], uniform((b, step, 0, 0), key, rules), rules)
        forced = fin[b] != 0 or (c["force"] is not None and 0 <= c["force"][b] <= step)
        tok = c["stop"] if forced else r["token"]
        if forced:
            r["arms"].add("forced")
        if step > cap:
            r["arms"].add("hist-capped")
        if step < cap:
            out_hist[b, step] = -1 if tok is None else tok
        if tok == c["stop"] and fin[b] == 0:
            fin[b] = 1
            state[2] += 1
        tokens.append(tok)
        rows.append(r)
        arms |= r["arms"]
        worst = min(worst, r["margin"])
    if not no_advance:
        state[0] += 1
        state[1] += 1
    return dict(tokens=tokens, history=out_hist, finished=fin, state=state, dbg=np.stack([r["dbg"] for r in rows]), rows=rows,
                arms=arms, margin=worst)


# ------------------------------------------------------------------------------------------------------------------ beam
def beam_row(lg, ids, c, rules=()):
    """Phase 1 of itts_beam_step for one row: float64 scores with their budgets, the kept candidates sorted.  Returns dict: s, w, gid
    (per kept candidate), ids, arms, margin."""
    V, nb = lg.shape[0], c["nb"]
    x = lg.astype(F64)
    mx = x.max()
    ex = np.exp(x - mx)
    se = ex.sum()
    lse = mx + math.log(se)
    with np.errstate(invalid="ignore"):
        E = float((ex * np.where(ex > 0, np.abs(x - mx) * EPS + 2 * U_EXP * EPS, 0.0)).sum() / se)
    A = 41 * EPS + E + 2 * U_LOG * EPS * abs(math.log(se)) + EPS * abs(lse)
    v = x - lse
    w = A + EPS * np.abs(v)
    pen = np.zeros(V, dtype=bool)
    arms = set()
    rep = F64(F32(c["rep"]))
    if F32(c["rep"]) != F32(1.0):
        pid, a = penalty_ids(ids, V, rules)
        arms |= {"b:" + x_ for x_ in a}
        for chunk in ([pid] if "dup-penalised-twice" not in rules else [pid[i:i + 1] for i in range(pid.shape[0])]):
            f = np.where(v[chunk] < 0, rep, 1.0 / rep)
            v[chunk] = v[chunk] * f
            w[chunk] = w[chunk] * f + EPS * np.abs(v[chunk])
        pen[pid] = True
    warp = bool(c["do_sample"])
    if warp and F32(c["temp"]) != F32(1.0):
        t = F64(F32(c["temp"]))
        v = v / t
        w = w / t + EPS * np.abs(v)
    w[~np.isfinite(v)] = 0.0
    gid = lg.astype(F32).view(np.uint32).astype(np.int64) * 2 + pen
    kk = min(max(int(c["top_k"]), 2) if warp else 2 * nb, V, MAXC)
    allid = np.arange(V)
    order = sort_order(v, allid, rules)
    kth = v[order[kk - 1]]
    n = kk if "kth-tie-dropped" in rules else int((v >= kth).sum())
    assert n <= MAXC, "a beam row with more than 1024 scores tied at the k-th value is outside the table"
    arms |= {"b:" + x_ for x_ in route(v.astype(F32), kk)}
    arms.add("b:search" if not warp else ("b:top_p<1" if F32(c["top_p"]) < F32(1.0) else "b:top_p=1"))
    chain = order[: min(n + 1, V)]                                   # the kept list and the first score below it
    worst = order_margin(v[chain], w[chain], gid[chain], None)
    kept = order[:n]
    keep = n
    if warp:
        mk = 1 if "beam-min-keep-1" in rules else 2
        keep, _, m2 = tail(v[kept], w[kept], float(F32(c["top_p"])), 0.0, mk, rules, draw=False)
        worst = min(worst, m2)
        if keep == 2 and n > 2 and F32(c["top_p"]) < F32(1.0):
            arms.add("b:min-keep-2")
    else:
        keep = min(n, 2 * nb)
    kept = kept[:keep]
    return dict(s=v[kept], w=w[kept], gid=gid[kept], ids=kept, arms=arms, margin=worst)


def order_margin(s, w, gid, exact):
    """Worst gap / budget over the neighbours of a list sorted descending.  An exact tie (same gid, or both entries exact fp32
    values) is decided by the index: no budget needed."""
    worst = INF
    for i in range(s.shape[0] - 1):
        if s[i] == s[i + 1]:
            tie_ok = gid[i] == gid[i + 1] or (exact is not None and exact[i] and exact[i + 1]) or not np.isfinite(s[i])
            if not tie_ok:
                return 0.0
        else:
            worst = min(worst, ratio(s[i] - s[i + 1], w[i] + w[i + 1]))
    return worst


def beam_case(c, rules=()):
    """One launch of itts_beam_step from the state the case uploads.  Returns the expected outputs and, for the values compared
    within a budget (beam_scores, hyp_score, worst), the budgets as `*_w`."""
    B, nb, cap, k, eos = c["B"], c["nb"], c["hist"].shape[2], c["step"], c["eos"]
    lg = c["lg"]
    R, V = lg.shape
    hin = c["hist"][k & 1]
    hist = c["hist"].copy()
    hout = hist[(k + 1) & 1]
    o = dict(tokens=np.zeros(R, np.int64), src=np.zeros(R, np.int64), beam_scores=c["beam_scores"].astype(F64), beam_scores_w=np.zeros(R),
             hyp_score=c["hyp_score"].astype(F64), hyp_score_w=np.zeros((B, nb)), hyp_len=c["hyp_len"].copy(), hyp_tok=c["hyp_tok"].copy(),
             n_hyp=c["n_hyp"].copy(), worst=c["worst"].astype(F64), worst_w=np.zeros(B), done=c["done"].copy(), cand_n=np.zeros(R, np.int64))
    state = np.array([k + 1, c["pos"] + 1, 0, 0, c["s45"][0], c["s45"][1], 0, 0], dtype=np.int64)
    key = philox_key(c["seed"], c["s45"][0], c["s45"][1], rules)
    arms, margin = set(), INF
    nhw = min(k, cap)
    if k == 0:
        arms.add("b:step0")
    if k >= cap:
        arms.add("b:hist-capped")
    lp = float(F32(c["lp"]))
    gen = float(k + 1)
    lp_div = 1.0 if lp == 0.0 else gen ** lp
    pw = 0.0 if lp == 0.0 else 2 * U_POW * EPS
    for b in range(B):
        sl = slice(b * nb, (b + 1) * nb)
        if c["done"][b]:
            arms.add("done-row")
            o["tokens"][sl], o["src"][sl], o["beam_scores"][sl] = eos, b * nb, 0.0
            nx_src, nx_tok = [0] * nb, [eos] * nb
        else:
            ps, pw_, pg, pf, prow = [], [], [], [], []
            for beam in range(nb):
                row = b * nb + beam
                ids = np.concatenate([c["extra"], hin[row, :nhw]])
                r = beam_row(lg[row], ids, c, rules)
                arms |= r["arms"]
                margin = min(margin, r["margin"])
                o["cand_n"][row] = r["ids"].shape[0]
                bsc = F32(c["beam_scores"][row])
                with np.errstate(over="ignore"):
                    lo = (np.clip(r["s"] - r["w"], -3e38, 3e38).astype(F32) + bsc).astype(F64)
                    hi = (np.clip(r["s"] + r["w"], -3e38, 3e38).astype(F32) + bsc).astype(F64)
                ex = (lo == hi) | ~np.isfinite(r["s"])
                P = np.where(np.isfinite(r["s"]), np.where(ex, lo, r["s"] + F64(bsc)), r["s"])
                ps.append(P)
                pw_.append(np.where(ex, 0.0, r["w"] + EPS * np.abs(P)))
                pg.append(np.where(ex, -1, r["gid"] + (row << 34)))
                pf.append(beam * V + r["ids"])
                prow.append(ex)
            ps, pw_, pg, pf, pex = (np.concatenate(a) for a in (ps, pw_, pg, pf, prow))
            if ps.shape[0] > MAXC:
                arms.add("pool-cut")
            if "pool-cut-after-sort" not in rules:
                ps, pw_, pg, pf, pex = (a[:MAXC] for a in (ps, pw_, pg, pf, pex))
            order = sort_order(ps, pf, rules)[:MAXC]
            ps, pw_, pg, pf, pex = (a[order] for a in (ps, pw_, pg, pf, pex))
            margin = min(margin, order_margin(ps, pw_, pg, pex))
            npool = ps.shape[0]
            want = min(2 * nb, npool)
            if c["do_sample"]:
                d = ps - ps[0]
                e = np.exp(d)
                with np.errstate(invalid="ignore"):
                    delta = np.where(e > 0, np.where(d == 0, 0.0, np.abs(d) * EPS + 2 * U_EXP * EPS) + pw_ + pw_[0], 0.0)
                alive = np.ones(npool, dtype=bool)
                picks = []
                for i in range(want):
                    u = F64(uniform((b, k, i, 0), key, rules))
                    ea = np.where(alive, e, 0.0)
                    total = ea.sum()
                    if total == 0.0:                                  # u * 0 = 0 and no running sum exceeds it: last live entry
                        arms.add("draw-fallback")
                        pick = int(np.nonzero(alive)[0][-1])
                    else:
                        run = np.cumsum(ea) / total
                        hit = np.nonzero(run > u)[0]
                        pick = int(hit[0]) if hit.shape[0] else int(np.nonzero(alive)[0][-1])
                        E2 = float((ea * delta).sum() / total)
                        j = np.arange(0, pick + 1 if hit.shape[0] else npool)
                        budget = run[j] * (j + 1) * EPS + u * (npool + 1) * EPS + 2 * E2
                        margin = min(margin, float(np.min(np.abs(run[j] - u) / budget)))
                    alive[pick] = False
                    picks.append(pick)
                picks = sorted(picks, key=lambda j_: (-ps[j_], picks.index(j_)))
            else:
                picks = list(range(want))
            hs_v = list(o["hyp_score"][b])
            hs_w = [0.0] * nb
            nh, worst, worst_w = int(c["n_hyp"][b]), float(o["worst"][b]), 0.0
            best = max(ps[j] for j in picks)
            nxt = []
            for rank, j in enumerate(picks):
                if len(nxt) >= nb:
                    break
                beam, tok, sc = int(pf[j] // V), int(pf[j] % V), float(ps[j])
                if tok == eos:
                    if (rank > nb) if "eos-rank-off-by-one" in rules else (rank >= nb):
                        arms.add("eos-low-rank-dropped")
                        continue
                    hs = sc / lp_div
                    hw = pw_[j] / lp_div + abs(hs) * (EPS + pw)
                    if nh >= nb:
                        margin = min(margin, ratio(abs(hs - worst), hw + worst_w))
                    if nh < nb or hs > worst:
                        if nh < nb:
                            slot = nh
                            nh += 1
                            arms.add("eos-closes")
                        else:
                            slot = int(np.argmin(hs_v))           # lowest score, earliest slot
                            srt = np.argsort(hs_v, kind="stable")
                            margin = min(margin, ratio(hs_v[srt[1]] - hs_v[srt[0]], hs_w[srt[1]] + hs_w[srt[0]]))
                            arms.add("evict-worst")
                        hs_v[slot], hs_w[slot] = hs, hw
                        o["hyp_len"][b, slot] = k
                        o["hyp_tok"][b, slot, :nhw] = hin[b * nb + beam, :nhw]
                        wi = int(np.argmin(hs_v[:nh]))
                        worst, worst_w = hs_v[wi], hs_w[wi]
                    else:
                        arms.add("eos-worse")
                else:
                    nxt.append((tok, beam, sc, pw_[j]))
            if len(nxt) < nb:
                arms.add("fill-from-first-beam")
            while len(nxt) < nb:
                nxt.append((nxt[0][0], nxt[0][1], -1e9, 0.0) if nxt else (eos, 0, -1e9, 0.0))
            o["hyp_score"][b], o["hyp_score_w"][b] = hs_v, hs_w
            o["n_hyp"][b], o["worst"][b], o["worst_w"][b] = nh, worst, worst_w
            if nh >= nb:
                margin = min(margin, ratio(abs(worst - best / lp_div), worst_w + abs(best / lp_div) * (2 * EPS + pw) + float(pw_.max()) / lp_div))
                if worst >= best / lp_div:
                    o["done"][b] = 1
                    state[2] += 1
                    arms.add("becomes-done")
            for i, (tok, beam, sc, w_) in enumerate(nxt):
                o["tokens"][b * nb + i], o["src"][b * nb + i] = tok, b * nb + beam
                o["beam_scores"][b * nb + i], o["beam_scores_w"][b * nb + i] = sc, w_
            nx_src, nx_tok = [t[1] for t in nxt], [t[0] for t in nxt]
        for i in range(nb):
            hout[b * nb + i, :nhw] = hin[b * nb + nx_src[i], :nhw]
            if k < cap:
                hout[b * nb + i, k] = nx_tok[i]
    o.update(hist=hist, state=state, arms=arms, margin=margin)
    return o


def arms(case):
    """The set of kernel arms a case of either table takes: the host mirror of the kernels' branch conditions (`route` for the top-k
    threshold over the thread-strided layout; the rest is collected where the reference takes the same branch)."""
    return (beam_case(case) if "nb" in case else sample_case(case))["arms"]


def kv_rows_ref(tbl, src, k1, P):
    """itts_beam_kv_rows: table k1 & 1 written from table (k1 + 1) & 1."""
    out = tbl.copy()
    _, R, smax = tbl.shape
    for r in range(R):
        out[k1 & 1, r, : min(P, smax)] = tbl[(k1 + 1) & 1, src[r], : min(P, smax)]
        if P < smax:
            out[k1 & 1, r, P] = r
    return out


# ------------------------------------------------------------------------------------------------------------------ case table
def two_rows(V, seed):
    """Row 0 peaked (sigma 3, the best token 4 above the next), row 1 flat (sigma 0.3)."""
    rng = np.random.default_rng(seed)
    lg = np.stack([rng.standard_normal(V) * 3.0, rng.standard_normal(V) * 0.3]).astype(F32)
    lg[0, int(np.argmax(lg[0]))] += F32(4.0)
    return lg


def tie_at(lg_row, rank, count):
    """Make the scores of ranks rank .. rank + count - 1 (0-based, descending) equal to the one at `rank - 1`."""
    order = np.argsort(-lg_row, kind="stable")
    lg_row[order[rank: rank + count]] = lg_row[order[rank - 1]]


def quantised(V, seed, residues=(3, 77)):
    """Steps of 0.5: thousands of scores at 1.0, and 32 higher ones per residue, all owned by the threads `residues` -- the kk-th
    largest per-thread maximum is 1.0 for any kk > len(residues), far more than 1024 scores pass that bound, and the exact k-th
    value (among the planted ones, 8 tied per level) is reached by a few."""
    rng = np.random.default_rng(seed)
    lg = rng.choice(np.array([0.0, 0.5, 1.0], dtype=F32), size=V, p=[0.3, 0.3, 0.4])
    for r in residues:
        i = np.arange(32)
        lg[r + 256 * i] = F32(2.0) + F32(0.5) * (i % 8 if r == residues[0] else i % 4)
    return lg.astype(F32)


def _s(name, lg, arms, pad=0, cap=8, step=0, hist=None, extra=(), rep=1.0, temp=1.0, top_k=30, top_p=1.0, do_sample=True,
       seed=1234, s45=(0, 0), finished=None, force=None, stop=None, pos=100):
    B, V = lg.shape
    rng = np.random.default_rng(V + step)
    return dict(name=name, lg=np.ascontiguousarray(lg, dtype=F32), pad=pad, step=step, pos=pos, extra=np.array(extra, dtype=np.int32),
                hist=(rng.integers(0, V, size=(B, cap)) if hist is None else np.array(hist)).astype(np.int32), rep=rep, temp=temp,
                top_k=top_k, top_p=top_p, do_sample=do_sample, seed=seed, s45=s45, finished=[0] * B if finished is None else finished,
                force=force, stop=V - 1 if stop is None else stop, arms=set(arms))


def sampler_cases():
    C = []
    one = np.array([[0.25]], dtype=F32)
    C.append(_s("V1 k30 p.8 t.7", one, {"fast", "tail<=64", "top_p<1", "keep=1"}, temp=0.7, top_p=0.8, stop=5))
    C.append(_s("V2 k2 p1 t1.3 ldl+3", two_rows(2, 1), {"fast", "tail<=64", "top_p=1"}, pad=3, temp=1.3, top_k=2, stop=5))
    C.append(_s("V255 k256 p.3", two_rows(255, 2), {"fast", "tail>64", "top_p<1", "keep=1"}, top_k=256, top_p=0.3))
    C.append(_s("V256 k257 p1 ldl+3", two_rows(256, 3), {"fast", "tail>64", "top_p=1"}, pad=3, top_k=257))
    C.append(_s("V257 k257 p.8 ldl+3", two_rows(257, 4), {"bisect", "tail>64", "top_p<1"}, pad=3, top_k=257, top_p=0.8, temp=1.3))
    C.append(_s("V1000 k1024 p.8 t.7", two_rows(1000, 61), {"bisect", "tail>64", "top_p<1", "keep=1"}, top_k=1024, top_p=0.8, temp=0.7))
    lg = two_rows(8194, 6)
    tie_at(lg[0], 30, 1)
    h = np.tile(np.argsort(-lg, axis=1)[:, :1], (1, 8))                 # the best token is in the history: the penalty moves it
    h[:, 1] = np.argsort(-lg, axis=1)[:, 3]
    C.append(_s("V8194 k30 p.8 t.7 rep10 step3", lg, {"fast", "fast-trim", "tail<=64", "top_p<1", "penalty-dup"}, step=3, hist=h, extra=(1, 8192), rep=10.0,
                temp=0.7, top_p=0.8))
    C.append(_s("V8448 k30 p.3 t1.3 ldl+3", two_rows(8448, 7), {"fast", "fast-trim", "tail<=64", "top_p<1", "keep=1"}, pad=3, temp=1.3, top_p=0.3))
    C.append(_s("V8194 k1 p.8", two_rows(8194, 8), {"fast", "tail<=64", "top_p<1", "keep=1"}, top_k=1, top_p=0.8))
    C.append(_s("V8194 k2 p1e-6", two_rows(8194, 9), {"fast", "tail<=64", "top_p<1", "keep=1"}, top_k=2, top_p=1e-6))
    C.append(_s("V8194 k64 p1: kept 64 by top_k", two_rows(8194, 10), {"fast", "fast-trim", "tail<=64", "top_p=1"}, top_k=64))
    C.append(_s("V8194 k65 p1: kept 65 by top_k", two_rows(8194, 11), {"fast", "fast-trim", "tail>64", "top_p=1"}, top_k=65))
    lg = two_rows(8194, 12)
    tie_at(lg[0], 60, 4)
    tie_at(lg[1], 60, 4)
    C.append(_s("V8194 k60 + 4 tied: kept 64", lg, {"fast", "fast-trim", "tail<=64", "top_p<1", "keep=1"}, top_k=60, top_p=0.8))
    lg = two_rows(8194, 13)
    tie_at(lg[0], 60, 5)
    tie_at(lg[1], 60, 5)
    C.append(_s("V8194 k60 + 5 tied: kept 65", lg, {"fast", "fast-trim", "tail>64", "top_p<1", "keep=1"}, top_k=60, top_p=0.8))
    # (k = 256: the bound is the LOWEST per-thread maximum, which thousands of scores reach)
    C.append(_s("V8194 k256 p.8 t.7", two_rows(8194, 14), {"overflow-bisect", "tail>64", "top_p<1", "keep=1"}, top_k=256, top_p=0.8, temp=0.7))
    C.append(_s("V8194 k257 p.3", two_rows(8194, 15), {"bisect", "tail>64", "top_p<1", "keep=1"}, top_k=257, top_p=0.3))
    C.append(_s("V8194 k1024 p1 t1.3", two_rows(8194, 16), {"bisect", "tail>64", "top_p=1"}, top_k=1024, temp=1.3))
    C.append(_s("V8194 k1024 p.8: the cut over 1024", two_rows(8194, 45), {"bisect", "tail>64", "top_p<1", "keep=1"}, top_k=1024, top_p=0.8))
    q = np.stack([quantised(8194, 18), quantised(8194, 19, residues=(200, 9))])
    C.append(_s("V8194 k30 steps of 0.5", q, {"overflow-bisect", "tail<=64", "top_p<1"}, top_p=0.8, temp=0.7))
    C.append(_s("V8194 k30 all equal p1", np.full((2, 8194), 1.5, dtype=F32), {"overflow-bisect", "overflow"}))
    C.append(_s("V8194 k4, 4 tied, p.5: cut ON the edge", _top_tied(8194, 20, 4), {"fast", "tail<=64", "top_p<1"}, top_k=4, top_p=0.5))
    lg = np.full((2, 1000), -np.inf, dtype=F32)
    lg[0, [5, 300, 301, 700, 999]] = [1.0, 2.5, 2.5, -0.5, 0.75]
    lg[1, [0, 255, 256, 512, 998]] = [0.1, 0.2, 0.3, 0.4, 0.5]
    C.append(_s("V1000 k30 five finite among -inf p.8", lg, {"fast", "fast-trim", "tail>64", "top_p<1"}, top_p=0.8))
    C.append(_s("V1000 k30 five finite among -inf p1", lg, {"fast", "fast-trim", "tail>64", "top_p=1"}))
    # the repetition penalty's corners: hist_cap 4 at row step 6 (window = 4 ids, nothing appended); ids outside [0, V) in the extra
    # ids and in the history; one id in both; a repeated id; a penalised score of exactly 0 and a negative one
    lg = two_rows(1000, 21)
    best = np.argsort(-lg, axis=1)
    lg[0, 17] = 0.0
    lg[1, best[1, 0]] = F32(-0.125)
    lg[1, best[1, 1]] = F32(-0.25)
    h = np.array([[best[0, 0], 17, 1000, best[0, 0]], [best[1, 0], -3, 40, 40]])
    for temp, do_sample, what in ((1.3, True, "sampled"), (0.7, False, "greedy ignores t.7")):
        C.append(_s(f"V1000 penalty corners cap4 step6 {what}", lg, ({"fast", "fast-trim", "tail<=64", "top_p<1"} if do_sample else {"greedy"}) |
                    {"penalty-dup", "penalty-out-of-range", "penalty-zero", "hist-capped"}, cap=4, step=6, hist=h,
                    extra=(int(best[0, 0]), 1, 8192, -1, int(best[1, 0])), rep=10.0, temp=temp, top_p=0.8, do_sample=do_sample))
    lg = two_rows(8194, 22)
    lg[0, 4000] = lg[0, 7000] = lg[0].max()                              # three equal maxima: the lowest id wins
    C.append(_s("V8194 greedy t.7 tied maxima ldl+3", lg, {"greedy"}, pad=3, temp=0.7, do_sample=False, top_k=1))
    lg = np.tile(two_rows(8194, 23)[1:] * F32(4.0), (4, 1))
    lg[0, 8193] = 50.0                                                   # row 0 draws the stop token, row 1 is stopped, row 2 had finished
    C.append(_s("V8194 k30 stop / force_stop / finished", lg, {"fast", "fast-trim", "tail<=64", "top_p<1", "forced", "keep=1"}, step=2, top_p=0.8,
                force=[-1, 2, -1, 5], finished=[0, 0, 1, 0], stop=8193))
    # one fixed row under 32 (seed, stream, step) triples: 4 launches x 8 rows; the seeds straddle 2^32, partly held in state[4..5]
    row = np.tile((np.random.default_rng(24).standard_normal(1000)).astype(F32), (8, 1))
    for seed, s45, step in ((2 ** 32 - 5, (9, 0), 0), (2 ** 32 + 7, (0, 0), 1), (2 ** 63 + 3, (M32, 0x7FFFFFFF), 5), (123, (0xFFFFFFF0, 1), 1000)):
        C.append(_s(f"V1000 k30 philox seed {seed:#x} + {s45[0]:#x}:{s45[1]:#x} step {step}", row, {"fast", "tail<=64", "top_p=1"} |
                    ({"hist-capped"} if step > 8 else set()), step=step, seed=seed, s45=s45))
    return C


def _top_tied(V, seed, count):
    lg = two_rows(V, seed)
    for r in lg:
        r[np.argsort(-r, kind="stable")[:count]] = r.max()
    return lg


def _b(name, lg, nb, arms, pad=0, cap=8, step=0, rep=1.0, temp=1.0, top_k=30, top_p=1.0, do_sample=True, lp=0.0, seed=77, s45=(0, 0),
       eos=None, beam_scores=None, hyp_score=None, n_hyp=None, worst=None, done=None, extra=(1,), hist_in=None, pos=40):
    R, V = lg.shape
    B = R // nb
    rng = np.random.default_rng(R * 1000 + V + step)
    hist = np.full((2, R, cap), -7, dtype=np.int32)
    hist[step & 1] = rng.integers(0, V, size=(R, cap)) if hist_in is None else hist_in
    if beam_scores is None:
        beam_scores = np.zeros((B, nb), dtype=F32)
        beam_scores[:, 1:] = -1e9 if step == 0 else -(np.arange(1, nb, dtype=F32) * F32(0.37))
    return dict(name=name, B=B, nb=nb, lg=np.ascontiguousarray(lg, dtype=F32), pad=pad, step=step, pos=pos, extra=np.array(extra, dtype=np.int32),
                hist=hist, rep=rep, temp=temp, top_k=top_k, top_p=top_p, do_sample=do_sample, lp=lp, seed=seed, s45=s45,
                eos=V - 1 if eos is None else eos, beam_scores=np.asarray(beam_scores, dtype=F32).reshape(R),
                hyp_score=np.zeros((B, nb), dtype=F32) if hyp_score is None else np.asarray(hyp_score, dtype=F32),
                hyp_len=np.zeros((B, nb), dtype=np.int32), hyp_tok=np.full((B, nb, cap), -9, dtype=np.int32),
                n_hyp=np.zeros(B, dtype=np.int32) if n_hyp is None else np.asarray(n_hyp, dtype=np.int32),
                worst=np.full(B, 1e9, dtype=F32) if worst is None else np.asarray(worst, dtype=F32),
                done=np.zeros(B, dtype=np.int32) if done is None else np.asarray(done, dtype=np.int32), arms=set(arms))


def spaced(R, V, seed, top, step=0.05, shift=True):
    """Rows whose `top` best logits are a permutation-placed ladder of `step`, the rest 12 below.  Pool entries of different rows
    are kept apart by shifting row r by r * step / (R + 1), or (shift=False) by the case's beam scores."""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((R, V)) * 0.2 - 12.0).astype(F32)
    for r in range(R):
        ids = rng.permutation(V - 1)[:top]                               # (never the last id: the EOS of these cases)
        lg[r, ids] = (-np.arange(top) * step + (r * step / (R + 1) if shift else 0.0)).astype(F32)
    return lg


def beam_cases():
    C = []
    rng = np.random.default_rng(31)
    C.append(_b("B3 nb3 V8194 k30 p.8 t.9 rep10 step0 sample", (np.random.default_rng(315).standard_normal((9, 8194)) * 2.5).astype(F32), 3,
                {"b:fast", "b:fast-trim", "b:top_p<1", "b:step0"}, cap=16, rep=10.0, temp=0.9, top_p=0.8, extra=(1, 8192)))
    lg = (rng.standard_normal((2, 50)) * 2.0).astype(F32)
    hin = rng.integers(0, 50, size=(2, 8))
    hin[0, 1] = hin[0, 0]
    C.append(_b("B1 nb2 V50 k1->2 p1 lp1 step3 ldl+3 sample", lg, 2, {"b:fast", "b:top_p=1", "b:penalty-dup", "b:penalty-out-of-range"}, pad=3, step=3,
                rep=10.0, top_k=1, lp=1.0, hist_in=hin, extra=(1, 8192, -2)))
    lg = spaced(8, 8194, 32, 128, shift=False)
    lg[5, np.argsort(-lg[5], kind="stable")[128]] = lg[5, np.argsort(-lg[5], kind="stable")[127]]   # beam 5 keeps 129: the pool holds 1025
    # The last beam is 25 ahead of the others and its 128 candidates lie within 0.26 of each other: every draw takes one of them
    # (each holds ~1/128 of the pool's mass, far more than a 1024-term fp32 sum can blur), and the one the cut drops -- its 128th --
    # is as likely as any other: a pool cut anywhere else changes the draws.
    top7 = np.argsort(-lg[7], kind="stable")[:128]
    lg[7, top7] = (-np.arange(128) * 0.002).astype(F32)
    bs = -(np.arange(8, dtype=F32) * F32(0.0045)) - F32(25.0)
    bs[7] = 0.0
    C.append(_b("B1 nb8 V8194 k128 p1 step2: a tie fills the pool past 1024", lg, 8, {"b:fast", "b:fast-trim", "b:top_p=1", "pool-cut"},
                step=2, top_k=128, temp=1.3, beam_scores=bs[None], seed=81))
    C.append(_b("B1 nb2 V8194 k2 p.3 t1.3 step4 sample", (rng.standard_normal((2, 8194)) * 2.5).astype(F32), 2,
                {"b:fast", "b:top_p<1"}, step=4, top_k=2, top_p=0.3, temp=1.3, rep=10.0))
    C.append(_b("B1 nb3 V8194 k30 p.3 step1 sample: top-p stops at 2", (rng.standard_normal((3, 8194)) * 4.0).astype(F32), 3,
                {"b:fast", "b:fast-trim", "b:top_p<1", "b:min-keep-2"}, step=1, top_p=0.3, seed=2 ** 32 - 1, s45=(5, 0)))
    q = np.stack([quantised(8194, 33), quantised(8194, 34, residues=(10, 20))])
    C.append(_b("B1 nb2 V8194 k30 steps of 0.5 sample", q, 2, {"b:overflow-bisect", "b:top_p<1"}, step=1, top_p=0.8))
    # beam search, V = 50, hist_cap 4 <= step 5.  Element 0: beam 0's best token is the EOS -> closes a hypothesis in a free slot;
    # element 1 had finished; element 2 has no EOS among its picks.
    lg = spaced(9, 50, 35, 12, step=0.3)
    lg[0, 49] = 1.0
    C.append(_b("B3 nb3 V50 search lp1 cap4 step5: EOS closes | done | plain", lg, 3, {"b:fast", "b:search", "b:hist-capped", "b:penalty-dup", "eos-closes", "done-row"},
                cap=4, step=5, do_sample=False, lp=1.0, rep=1.2, done=[0, 1, 0]))
    # Element 0, full store: the EOS hypothesis beats the worst (-30), which is evicted; element 1, full store: it does not (worst
    # -0.001), the store stays and the element becomes done; element 2: beam 0's EOS closes at rank 0, beam 1 (the same logits,
    # 1.3 behind) has its EOS at rank 3 >= num_beams -> dropped.
    lg = spaced(9, 50, 36, 12, step=0.3)
    lg[0, 49] = lg[3, 49] = lg[6, 49] = 1.0
    lg[7] = lg[6]
    bs = np.zeros((3, 3), dtype=F32)
    bs[:, 1:] = [-40.0, -50.0]
    bs[2, 1] = -1.3
    C.append(_b("B3 nb3 V50 search lp0 step2: evict | worse | low rank", lg, 3, {"b:fast", "b:search", "evict-worst", "eos-worse", "eos-closes",
                                                                                   "eos-low-rank-dropped", "becomes-done"},
                step=2, do_sample=False, beam_scores=bs, n_hyp=[3, 3, 0], worst=[-30.0, -0.001, 1e9],
                hyp_score=[[-20.0, -30.0, -25.0], [-0.001, -0.0005, -0.0002], [0, 0, 0]]))
    C.append(_b("B1 nb2 V1 search: the only token is the EOS", np.array([[0.5], [0.25]], dtype=F32), 2,
                {"b:fast", "b:search", "eos-closes", "fill-from-first-beam"}, step=1, do_sample=False, eos=0, extra=()))
    C.append(_b("B1 nb8 V50 k30 p.8 lp1 step0 sample", (rng.standard_normal((8, 50)) * 2.0).astype(F32), 8,
                {"b:fast", "b:top_p<1", "b:step0", "draw-fallback"}, top_p=0.8, lp=1.0, temp=0.9))
    C.append(_b("B1 nb2 V50 k2 p1 step0 sample: four draws from nothing", (rng.standard_normal((2, 50)) * 2.0).astype(F32), 2,
                {"b:fast", "b:top_p=1", "b:step0", "draw-fallback"}, top_k=2))
    return C


def kv_cases():
    C = []
    for rows, nb, smax, P, k1 in ((2, 2, 64, 0, 1), (2, 2, 64, 1, 2), (2, 2, 64, 63, 3), (24, 3, 257, 0, 2), (24, 3, 257, 1, 1), (24, 3, 257, 256, 4),
                                  (24, 8, 64, 40, 7)):
        rng = np.random.default_rng(rows * smax + P)
        tbl = rng.integers(0, rows, size=(2, rows, smax)).astype(np.int32)
        src = (np.arange(rows) // nb * nb + rng.integers(0, nb, size=rows)).astype(np.int32)
        src[:nb] = np.arange(nb)[::-1]                                     # rows of one batch element swap places
        C.append(dict(name=f"rows {rows} smax {smax} P {P} parity {k1 & 1}", tbl=tbl, src=src, k1=k1, P=P))
    return C
