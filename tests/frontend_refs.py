"""float64 references of the prompt front-end kernels (csrc/frontend.hip), their per-element error bounds and the operand
generators of tests/test_frontend_kernels_gpu.py.  Device-agnostic plain torch: every function works on the device of its
operands and makes no call into the library, so tests/test_frontend_refs_cpu.py can hold the references to torch's own float64
operators, and prove that every negative control leaves its bound, without a GPU.

A reference takes the operands as the kernel sees them (16-bit operands already rounded, fp32 parameters as they are), evaluates
the operation in float64 and rounds an intermediate to the storage type only where the kernel does, with an operation that is
bit-identical to the kernel's (`rsum`: IEEE fp32 add, then round-to-nearest-even to T; fp64_check.walk_step: the rounding of P in
mha_small -- the walk's step, `fold_rows` and `rnd` are the ones the decode file uses).
`exact=True` switches those roundings off (the CPU test's comparison with torch.softmax / F.conv1d).

Bounds (u = 2^-24; every bound is a tensor):
  ulp_T(ref)            the store to the 16-bit type (none for an fp32 output)
  (n + 1) u S           a chain of n fp32 additions / fmafs with magnitude sum S, where n is counted from the kernel
  2^-21 S               an MFMA chain or a long fmaf chain (the project's fp32-chain figure)
  (|x| + 2) u           relative error of __expf(x): one product with log2 e and the hardware exp2 (the decode file's figure)
  L                     the Lipschitz constant of a trailing activation: SiLU 1.10, ReLU 1, sigmoid 1/4
  LayerNorm behind a computed value: the input error goes through rstd |lw|, plus the relative error of rstd
  sqrt of a variance:   the variance error over the sum of the two roots, the kernel's root being at least 1e-6 (the 1e-12 clamp)
"""
import math

import torch

from fp64_check import fold_rows, rnd, ulp, walk_start, walk_step  # noqa: F401

U = 2.0 ** -24          # unit roundoff of fp32
CHAIN = 2.0 ** -21      # the project's fp32-chain figure (MFMA / long fmaf chains), relative to the magnitude sum
# Accuracy of the device library's erff in units of 2^-24, absolute on |erf| <= 1.  ROCm's math documentation is not part of the
# tree this was written against, so the figure is measured: the worst |erff(a) - erf(a)| over geglu_inputs' own gate grid
# (a = fp32(g * fp32(1/sqrt 2)), erf in float64) on an MI355X was ERF_MEASURED u (bf16 and f16 grids alike); C_ERF is twice that.  Both numbers are in the
# header of profiles/frontend_kernels_fp64.txt, and test_geglu prints the measurement of its run.
ERF_MEASURED = 0.957
C_ERF = 2.0 * ERF_MEASURED
POISON = 1000.0         # what the padding rows of every packed operand a kernel reads are filled with
SENT = 7.0              # sentinel of output buffers (finite, non-zero, exact in bf16 and f16)


def rsum(a, b, dtype, exact=False):
    """The kernel's `from_f(to_f(a) + b)`: an IEEE fp32 add, then round-to-nearest-even to T."""
    if exact:
        return a.double() + b.double()
    return (a.float() + b.float()).to(dtype).double()


# ---------------------------------------------------------------------------------------------- packed operand layout
def pack_padded(xp):
    """[mtp * 16][K] (padding rows included, whatever they hold) -> the flat packed 16-bit activation layout."""
    R, K = xp.shape
    return xp.view(R // 16, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)


def unpack_padded(flat, mtp, K):
    return flat.view(K // 32, mtp, 4, 16, 8).permute(1, 3, 0, 2, 4).contiguous().view(mtp * 16, K)


def padded(x, mtp, fill=POISON):
    """x [T][K] on top of padding rows that hold `fill`: [mtp * 16][K]."""
    out = torch.full((mtp * 16, x.shape[1]), fill, dtype=x.dtype, device=x.device)
    out[: x.shape[0]] = x
    return out


# ---------------------------------------------------------------------------------------------- subsample_conv
def subsample_conv_ref(mel, w, b, relu=True, row_shift=0):
    """relu(Conv2d(1, C, 3, stride 2)) of mel [T][F] as [T2][C * F2]; returns (ref, S) with S the magnitude sum of the chain.
    row_shift: the stride-2 window starts row_shift mel rows late (rows wrap: a control)."""
    T, F = mel.shape
    C = w.shape[0]
    T2, F2 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    md = torch.roll(mel.double(), -row_shift, 0) if row_shift else mel.double()
    wd, bd = w.double(), b.double()
    acc = bd[:, None, None].expand(C, T2, F2).clone()
    S = acc.abs()
    for i in range(3):
        for j in range(3):
            win = md[i: i + 2 * T2 - 1: 2, j: j + 2 * F2 - 1: 2]           # [T2][F2]
            acc = acc + wd[:, 3 * i + j, None, None] * win
            S = S + wd[:, 3 * i + j, None, None].abs() * win.abs()
    if relu:
        acc = torch.relu(acc)
    return acc.permute(1, 0, 2).reshape(T2, C * F2), S.permute(1, 0, 2).reshape(T2, C * F2)


def subsample_conv_bound(ref, S, dtype):
    """bias + nine fmafs in fp32 (n = 9), ReLU (L = 1), one store."""
    return ulp(ref, dtype) + 10 * U * S


def subsample_inputs(T, F, C, seed=100, device="cpu"):
    mel = rnd(T, F, seed=seed, scale=2.0, device=device).float()
    if T % 2 == 0:
        mel[T - 1] = POISON                      # an even T leaves the last mel row outside every window
    w = rnd(C, 9, seed=seed + 1, scale=0.3, device=device).float()
    b = rnd(C, seed=seed + 2, scale=0.3, device=device).float()
    b[-1] = 0.75
    return mel, w, b


# ---------------------------------------------------------------------------------------------- mha_small
def mha_small_ref(q, k, v, scale, pos=None, bu=None, bv=None, exact=False):
    """Form (a): q [Tq][H][64], k / v [Tk][H][64] (storage type), pos [H][Tk][64] or None, bu / bv fp32 [H * 64].
    Walks the keys as the kernel does -- 32-key steps dealt round-robin to four waves, a running maximum per wave,
    P = round_T(exp(s - m_step)), the normaliser sums the rounded P -- and merges the four states in float64.
    Returns (ref [Tq][H * 64], E, info): E is the fp32-level budget of `mha_small_bound`, info holds T_j, T_max, P_j (the float64
    softmax weights) and the near-midpoint flags, each [H][Tq][Tk], and E_flip, the part of E that the flagged weights contribute."""
    dtype = v.dtype
    Tq, H, _ = q.shape
    Tk = k.shape[0]
    dev = q.device
    kd, vd = k.double().transpose(0, 1), v.double().transpose(0, 1)                  # [H][Tk][64]
    if pos is not None:
        qu = rsum(q, bu.view(1, H, 64), dtype, exact).transpose(0, 1)                 # [H][Tq][64]
        qv = rsum(q, bv.view(1, H, 64), dtype, exact).transpose(0, 1)
        pd = pos.double()
        s = (qu @ kd.transpose(1, 2) + qv @ pd.transpose(1, 2)) * scale
        Tj = (qu.abs() @ kd.abs().transpose(1, 2) + qv.abs() @ pd.abs().transpose(1, 2)) * scale
    else:
        qd = q.double().transpose(0, 1)
        s = qd @ kd.transpose(1, 2) * scale
        Tj = qd.abs() @ kd.abs().transpose(1, 2) * scale
    Tmax = Tj.max(-1, keepdim=True).values
    delta = CHAIN * (Tj + Tmax) + 2.0 ** -19          # relative distance of the kernel's fp32 P_j from the float64 one
    states = []
    near_all = torch.zeros(H, Tq, Tk, dtype=torch.bool, device=dev)
    for wave in range(4):
        state = walk_start(H, Tq, dev)
        for kb in range(32 * wave, Tk, 128):
            state, near_all[:, :, kb:kb + 32] = walk_step(state, s[:, :, kb:kb + 32], delta[:, :, kb:kb + 32], vd[:, kb:kb + 32], dtype,
                                                          sum_rounded=True, exact=exact)
        states.append(state)
    M = torch.stack([st[0] for st in states]).max(0).values
    L, O, _, Em, Ed, dbar, nbar = (sum(torch.exp(st[0] - M) * st[i] for st in states) for i in range(1, 8))   # a wave without keys: m = -inf, weight 0
    out = lambda t: (t / L).transpose(0, 1).reshape(Tq, H * 64)  # noqa: E731
    ref = out(O)
    # a weight the kernel may round the other way moves the product by ulp_T(P_j) |v_j| and the normaliser by ulp_T(P_j)
    E = out(Em) + out(Ed) + (out(dbar.expand(H, Tq, 64)) + out(nbar.expand(H, Tq, 64))) * ref.abs()
    Pj = torch.softmax(s, -1)
    return ref, E, dict(T_j=Tj, T_max=Tmax, P_j=Pj, near=near_all, E_flip=out(Em) + out(nbar.expand(H, Tq, 64)) * ref.abs())


def mha_small_bound(ref, E, dtype):
    return ulp(ref, dtype) + E


def mha_oneshot(q, k, v, scale, pos=None, bu=None, bv=None):
    """One-shot float64 softmax attention, no intermediate rounding: what the walking reference must equal with exact=True."""
    Tq, H, _ = q.shape
    qd, kd, vd = (t.double().transpose(0, 1) for t in (q, k, v))
    if pos is None:
        s = qd @ kd.transpose(1, 2)
    else:
        s = (qd + bu.double().view(H, 1, 64)) @ kd.transpose(1, 2) + (qd + bv.double().view(H, 1, 64)) @ pos.double().transpose(1, 2)
    return (torch.softmax(s * scale, -1) @ vd).transpose(0, 1).reshape(Tq, H * 64)


def mha_controls(q, k, v, pos, bu, bv):
    """(name, reference under the control) of the mha_small family; the CPU and the GPU test share them."""
    Tk = k.shape[0]
    out = [("key Tk - 1 dropped", mha_small_ref(q, k[:-1], v[:-1], 0.125, pos[:, :-1], bu, bv)[0]),
           ("the clamped duplicate of key Tk - 1 admitted as key Tk",
            mha_small_ref(q, torch.cat([k, k[-1:]]), torch.cat([v, v[-1:]]), 0.125, torch.cat([pos, pos[:, -1:]], 1), bu, bv)[0])]
    vs = v.clone()
    vs[[0, 1]] = v[[1, 0]]
    out.append(("V rows 0 and 1 of a 32-key step exchanged", mha_small_ref(q, k, vs, 0.125, pos, bu, bv)[0]))
    out.append(("bias_u used in both terms", mha_small_ref(q, k, v, 0.125, pos, bu, bu)[0]))
    out.append(("the position term dropped", mha_small_ref(q, k, v, 0.125, torch.zeros_like(pos), bu, bv)[0]))
    assert Tk > 1
    return out


def mha_inputs(Tq, Tk, H, rel, dtype, seed=None, device="cpu"):
    """Scores with a standard deviation of about 2; the keys Tk - 1, 0 and every 4-key slot boundary 16 j + 4 g of every 32-key step
    (the first key of every step among them) score about 6 against every query: the queries share a common component c and the
    marked keys point along it.  Returns q, k, v [T][H][64], pos, bu, bv (None without the position term)."""
    seed = 200 + Tk if seed is None else seed
    c = rnd(1, H, 64, seed=seed, device=device)
    q = (c + 0.5 * rnd(Tq, H, 64, seed=seed + 1, device=device)).to(dtype)
    k = rnd(Tk, H, 64, seed=seed + 2, scale=1.5 if rel else 1.8, device=device)
    marks = sorted(set(range(0, Tk, 4)) | {Tk - 1})
    k[marks] = 0.05 * k[marks] + 48.0 * c / (c * c).sum(-1, keepdim=True)
    v = rnd(Tk, H, 64, seed=seed + 3, device=device).to(dtype)
    if not rel:
        return q, k.to(dtype), v, None, None, None
    pos = rnd(H, Tk, 64, seed=seed + 4, scale=0.8, device=device).to(dtype)
    bu = rnd(H * 64, seed=seed + 5, scale=0.2, device=device).float()
    bv = rnd(H * 64, seed=seed + 6, scale=0.2, device=device).float()
    return q, k.to(dtype), v, pos, bu, bv


# ---------------------------------------------------------------------------------------------- glu_dwconv_ln_silu
def glu_dwconv_ln_silu_ref(x, w, b, lw, lb, eps=1e-5, dtype=None, drop_tap=None, replicate=False, swap_halves=False, var_div=None):
    """x [T][2 C] (value | gate, storage type) -> GLU -> depthwise conv over time (zero "same" padding) -> LayerNorm -> SiLU.
    Returns (ref [T][C], bound) -- the bound needs `dtype`.  The keyword arguments are the negative controls."""
    T, C2 = x.shape
    C = C2 // 2
    KT = w.shape[1]
    h = (KT - 1) // 2
    xd = x.double()
    a, g = (xd[:, C:], xd[:, :C]) if swap_halves else (xd[:, :C], xd[:, C:])
    gl = a * torch.sigmoid(g)
    # the kernel: a / (1 + __expf(-g)): __expf (|g| + 2) u on a term that is at most 1 of the denominator, the add, the division
    gerr = gl.abs() * (g.abs() + 4.0) * U
    if replicate:
        glp = torch.cat([gl[:1].expand(h, C), gl, gl[-1:].expand(h, C)])
    else:
        glp = torch.cat([gl.new_zeros(h, C), gl, gl.new_zeros(h, C)])
    gep = torch.cat([gl.new_zeros(h, C), gerr, gl.new_zeros(h, C)])
    wd = w.double()
    c = b.double()[None].expand(T, C).clone()
    S, e = c.abs(), torch.zeros_like(c)
    for j in range(KT):
        if j == drop_tap:
            continue
        c = c + glp[j:j + T] * wd[:, j]
        S = S + (glp[j:j + T] * wd[:, j]).abs()
        e = e + gep[j:j + T] * wd[:, j].abs()
    e = e + (KT + 1) * U * S                                  # the chain of KT fmafs on top of the bias
    mean = c.mean(1, keepdim=True)
    d = c - mean
    var = (d * d).sum(1, keepdim=True) / (var_div or C)
    rstd = 1.0 / torch.sqrt(var + eps)
    lwd, lbd = lw.double(), lb.double()
    vv = d * rstd * lwd + lbd
    ref = vv * torch.sigmoid(vv)
    if dtype is None:
        return ref, None
    # LayerNorm behind a computed value: d carries e, the error of the mean (its inputs' mean error + a tree sum) and its own rounding;
    # the variance 2 mean(|d| e_d) + a tree sum; rstd half the relative variance error + rsqrtf (1 ulp) and the division by C
    e_mean = e.mean(1, keepdim=True) + CHAIN * c.abs().mean(1, keepdim=True)
    e_d = e + e_mean + U * d.abs()
    e_var = 2.0 * (d.abs() * e_d).mean(1, keepdim=True) + CHAIN * var
    d_r = 0.5 * e_var / (var + eps) + 3.0 * U
    e_v = rstd * lwd.abs() * e_d + (d_r + 3.0 * U) * (vv - lbd).abs() + U * vv.abs()
    # SiLU: L = 1.10 on the input error, and v / (1 + __expf(-v)) itself like the GLU above
    bound = ulp(ref, dtype) + 1.10 * e_v + (vv.abs() + 4.0) * U * ref.abs()
    return ref, bound


def glu_outlier_row(T, cls):
    """The middle row; with the classes dealt by thirds, the middle of the first third, whose window holds its own class alone."""
    return T // 2 if cls is not None else T // 6


def glu_inputs(T, C, taps, dtype, cls=None, seed=None, device="cpu"):
    """b carries a common offset of 4 and the value half's amplitude sets the conv output's sigma, so that |mean| / sigma is below 1
    (class 0), about 8 (class 1) or above 64 (class 2).  The convolution blends (taps - 1) / 2 rows on either side, so with a common
    b the class belongs to a window of rows, never to a single row: cls = None deals the classes by thirds of the rows (each exists
    where T / 3 > (taps - 1) / 2), cls = 0 / 1 / 2 puts every row of a shorter case into that class.  Channel 5 passes its own row
    alone (centre tap 1, the others 0) and row `glu_outlier_row` holds an outlier of 60 sigma there: one channel of the conv output of
    one row."""
    seed = 300 + T if seed is None else seed
    h = (taps - 1) // 2
    s0 = 0.1616 * math.sqrt(min(taps, T))                      # sigma of the conv output at amplitude 1: w 0.3, E[sigmoid^2] 0.29, the taps that see a row
    third = torch.clamp(torch.arange(T, device=device) * 3 // max(T, 1), max=2)
    if cls is not None:
        third = torch.full_like(third, cls)
    amp = (4.0 / s0 / torch.tensor([0.25, 8.0, 90.0], dtype=torch.float64, device=device))[third][:, None]
    x = rnd(T, 2 * C, seed=seed, device=device)
    x[:, :C] *= amp
    r = glu_outlier_row(T, cls)
    x[r, 5], x[r, C + 5] = 60.0 * s0 * float(amp[r]), 8.0
    w = rnd(C, taps, seed=seed + 1, scale=0.3, device=device).float()
    w[5], w[5, h] = 0.0, 1.0
    b = (4.0 + rnd(C, seed=seed + 2, scale=0.02, device=device)).float()
    lw = (1.0 + rnd(C, seed=seed + 3, scale=0.1, device=device)).float()
    lb = rnd(C, seed=seed + 4, scale=0.1, device=device).float()
    return x.to(dtype), w, b, lw, lb


# ---------------------------------------------------------------------------------------------- rows
def rows_ref(M, D, x=None, slab=None, bias=None, norm=0, w=None, b=None, eps=1e-5, drop_slab=None, bias_twice=False, no_mean=False,
             no_sqrt_d=False):
    """v = x + bias + slab[0] + ... (float64); norm 1 LayerNorm(w, b), norm 2 v / max(|v|_2, 1e-12) sqrt(D) w.
    Returns (ref [M][D], bound): the fp32 y gets no ulp term -- (nslab + 2) u S for the sum, then the norm's terms."""
    nslab = 0 if slab is None else slab.shape[0]
    dev = (x if x is not None else slab).device
    v = torch.zeros(M, D, dtype=torch.float64, device=dev)
    S = torch.zeros_like(v)
    if x is not None:
        v, S = v + x.double(), S + x.double().abs()
    if bias is not None:
        f = 2.0 if bias_twice else 1.0
        v, S = v + f * bias.double(), S + bias.double().abs()
    for s in range(nslab):
        if s == drop_slab:
            continue
        v, S = v + slab[s].double(), S + slab[s].double().abs()
    e = (nslab + 2) * U * S
    if norm == 0:
        return v, e + 1e-300
    wd = w.double()
    if norm == 1:
        mean = v.mean(1, keepdim=True) * (0.0 if no_mean else 1.0)
        d = v - mean
        var = (d * d).mean(1, keepdim=True)
        k = 1.0 / torch.sqrt(var + eps)
        ref = d * k * wd + b.double()
        e_mean = e.mean(1, keepdim=True) + CHAIN * v.abs().mean(1, keepdim=True)
        e_d = e + e_mean + U * d.abs()
        e_var = 2.0 * (d.abs() * e_d).mean(1, keepdim=True) + CHAIN * var
        d_k = 0.5 * e_var / (var + eps) + 3.0 * U                # + the division by D, the add of eps, rsqrtf
        return ref, k * wd.abs() * e_d + (d_k + 3.0 * U) * (d * k * wd).abs() + U * ref.abs() + 1e-300
    s2 = (v * v).sum(1, keepdim=True)
    k = (1.0 if no_sqrt_d else math.sqrt(D)) / torch.clamp(torch.sqrt(s2), min=1e-12)
    ref = v * k * wd
    e_s2 = 2.0 * (v.abs() * e).sum(1, keepdim=True) + CHAIN * s2
    d_k = 0.5 * e_s2 / torch.clamp(s2, min=1e-300) + 4.0 * U     # two square roots, the division
    return ref, k * wd.abs() * e + (d_k + 3.0 * U) * ref.abs() + 1e-300


def rows_inputs(M, D, nslab, norm, dtype=None, x=True, bias=True, special=None, device="cpu"):
    """x [M][D], slab [nslab][M][D], bias [D], and the norm's w / b (fp32; None where absent).  special "fold": x holds fold_rows
    rows; "zero": row M // 2 of x is zero.  The seed follows from the case, so every test of one case draws the same operands."""
    seed = 400 + 1000 * norm + 10 * nslab + D % 97 + M
    xs = fold_rows(M, D, seed, device=device).float() if special == "fold" else rnd(M, D, seed=seed, device=device).float()
    if special == "zero":
        xs[M // 2] = 0.0
    slab = rnd(nslab, M, D, seed=seed + 1, device=device).float() if nslab else None
    bs = rnd(D, seed=seed + 2, device=device).float() if bias else None
    w = (1.0 + 0.1 * rnd(D, seed=seed + 3, device=device)).float() if norm else None
    b = rnd(D, seed=seed + 4, scale=0.1, device=device).float() if norm == 1 else None
    return (xs if x else None), slab, bs, w, b


# ---------------------------------------------------------------------------------------------- geglu
def geglu_ref(h, dtype=None, swap_halves=False):
    """gelu(gate) * x (erf form) of h [M][2 Kp] (x | gate); returns (ref, bound)."""
    Kp = h.shape[1] // 2
    hd = h.double()
    x, g = (hd[:, Kp:], hd[:, :Kp]) if swap_halves else (hd[:, :Kp], hd[:, Kp:])
    ref = 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))) * x
    if dtype is None:
        return ref, None
    # 0.5 g (1 + erff(g c)) x: erff's absolute error C_ERF u and the argument's rounding (g c in fp32, c itself: at most
    # 1.5 u |a| erf'(a) <= u) both enter 1 + erf absolutely -- the cancellation tail keeps them --, then one addition and two products
    return ref, ulp(ref, dtype) + (C_ERF + 1.0) * U * 0.5 * (g * x).abs() + 4.0 * U * ref.abs()


def geglu_inputs(M, Kp, dtype, seed=None, device="cpu"):
    """x random; the gates walk a grid over [-6, 6] that holds 0 and the tail where 1 + erf cancels (gate < -5: 1 + erf < 2^-22)."""
    h = rnd(M, 2 * Kp, seed=500 + M if seed is None else seed, device=device)
    n = M * Kp
    grid = torch.linspace(-6.0, 6.0, 193, dtype=torch.float64, device=device)        # step 1/16: 0 is a grid point
    h[:, Kp:] = grid[(torch.arange(n, device=device) * 7) % 193].view(M, Kp)
    return h.to(dtype)


# ---------------------------------------------------------------------------------------------- im2col_reflect
def reflect_index(i, n, mode="reflect"):
    if mode == "replicate":
        return i.clamp(0, n - 1)
    if mode == "symmetric":                                   # the reflection that repeats the edge sample
        return torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))


def im2col_reflect_ref(x, taps, dil, Kp, mode="reflect"):
    """x fp32 [T][F] -> [T][Kp] float64: column j F + f = x[reflect(t + (j - (taps - 1) / 2) dil)][f], zeros from taps F on."""
    T, F = x.shape
    t = torch.arange(T, device=x.device)
    out = torch.zeros(T, Kp, dtype=torch.float64, device=x.device)
    for j in range(taps):
        out[:, j * F:(j + 1) * F] = x.double()[reflect_index(t + (j - (taps - 1) // 2) * dil, T, mode)]
    return out


def im2col_inputs(T, F, device="cpu"):
    return rnd(T, F, seed=600 + T, device=device).float()


# ---------------------------------------------------------------------------------------------- res2_step
def res2_step_ref(y1, cat, w, bias, scale, shift, s, dil, first, dtype, exact=False, mode="reflect", reverse_taps=False, add_prev=True,
                  no_shift=False):
    """Chunk s of one Res2Net step over y1 / cat [T][C] (storage type); w [64 out][64 in][3] already rounded to the storage type.
    Returns (ref [T][64], bound)."""
    T = y1.shape[0]
    a = y1[:, 64 * s:64 * s + 64]
    inp = a.double() if (first or not add_prev) else rsum(a, cat[:, 64 * s - 64:64 * s], dtype, exact)
    t = torch.arange(T, device=y1.device)
    wd = w.double()
    acc = torch.zeros(T, 64, dtype=torch.float64, device=y1.device)
    S = torch.zeros_like(acc)
    for j in range(3):
        rows = inp[reflect_index(t + (j - 1) * dil, T, mode)]
        wj = wd[:, :, 2 - j if reverse_taps else j]
        acc, S = acc + rows @ wj.t(), S + rows.abs() @ wj.abs().t()
    pre = acc + bias.double()
    S = S + bias.double().abs()
    sc = scale.double()
    ref = torch.relu(pre) * sc + (0.0 if no_shift else shift.double())
    # six chained 32-deep MFMAs and the bias, ReLU (L = 1), one fmaf, one store
    return ref, ulp(ref, dtype) + sc.abs() * (CHAIN * S + U * pre.abs()) + U * ref.abs()


def res2_inputs(T, dtype, device="cpu"):
    """y1, cat [T][512] and w [64][64][3] in the storage type, bias, BatchNorm scale and shift fp32 [64]."""
    y1, cat = rnd(T, 512, seed=700 + T, device=device).to(dtype), rnd(T, 512, seed=701 + T, device=device).to(dtype)
    w = rnd(64, 64, 3, seed=702, scale=0.08, device=device).to(dtype)
    b, sc = rnd(64, seed=703, scale=0.1, device=device).float(), (1 + 0.1 * rnd(64, seed=704, device=device)).float()
    return y1, cat, w, b, sc, rnd(64, seed=705, scale=0.3, device=device).float()


# ---------------------------------------------------------------------------------------------- se_gate
def se_gate_ref(y, w1, b1, w2, b2, mtp, rows=None, no_b1=False, relu=True):
    """gate = sigmoid(w2 relu(w1 mean_t(y) + b1) + b2); y [T][C], w1 [H][C], w2 [C][H] (storage type).  rows: the mean's
    divisor stays T while the sum runs over `rows` ([R][C], the padded operand: the guard's control).  Returns (ref [C], bound):
    fp32 output, no ulp term."""
    T = y.shape[0]
    yd = (y if rows is None else rows).double()
    mean = yd.sum(0) / T
    e_m = (mtp + 6) * U * yd.abs().sum(0) / T       # mtp additions per lane, four shuffle steps, the division
    w1d, w2d = w1.double(), w2.double()
    pre1 = w1d @ mean + (0.0 if no_b1 else b1.double())
    e_1 = CHAIN * (w1d.abs() @ mean.abs() + b1.double().abs()) + w1d.abs() @ e_m
    hid = torch.relu(pre1) if relu else pre1
    pre2 = w2d @ hid + b2.double()
    e_2 = CHAIN * (w2d.abs() @ hid.abs() + b2.double().abs()) + w2d.abs() @ e_1
    ref = torch.sigmoid(pre2)
    # sigmoid: L = 1/4; 1 / (1 + __expf(-x)): (|x| + 2) u on the exponential, the add, the division
    return ref, 0.25 * e_2 + (pre2.abs() + 4.0) * U * ref


def se_inputs(T, C, H, dtype, seed=None, device="cpu"):
    seed = 800 + T if seed is None else seed
    y = (rnd(T, C, seed=seed, device=device) + 0.5).to(dtype)
    w1 = rnd(H, C, seed=seed + 1, scale=2.0 * C ** -0.5, device=device).to(dtype)
    b1 = rnd(H, seed=seed + 2, scale=0.5, device=device).float()
    w2 = rnd(C, H, seed=seed + 3, scale=2.0 * H ** -0.5, device=device).to(dtype)
    b2 = rnd(C, seed=seed + 4, scale=0.5, device=device).float()
    return y, w1, b1, w2, b2


# ---------------------------------------------------------------------------------------------- scale_resid
def scale_resid_ref(y, res, gate, dtype, gate_shift=0):
    """gate[c] y + res: one fmaf, one store."""
    g = torch.roll(gate.double(), gate_shift) if gate_shift else gate.double()
    ref = g * y.double() + res.double()
    return ref, ulp(ref, dtype) + U * ref.abs()


def scale_resid_inputs(T, C, dtype, device="cpu"):
    """y, res [T][C] in the storage type and the fp32 gate [C]."""
    return (rnd(T, C, seed=850 + T, device=device).to(dtype), rnd(T, C, seed=851 + T, device=device).to(dtype),
            torch.sigmoid(rnd(C, seed=852, device=device)).float())


# ---------------------------------------------------------------------------------------------- col_stats
def col_stats_ref(x, mtp, dtype, logit=None, scale=None, shift=None, uniform=False, var_div_t1=False, shift_low=False):
    """[m | s] (* scale + shift) over the rows of x [T][C] (storage type), weights softmax_t(logit) or 1 / T.
    Returns (ref [2 C], bound).  n = ceil(mtp / 8) + 12 additions at most: a lane's blocks, four shuffle steps, eight LDS rows."""
    T, C = x.shape
    xd = x.double()
    n = -(-mtp // 8) + 12
    if logit is not None and not uniform:
        ld = logit.double()
        dl = (ld - ld.max(0, keepdim=True).values).abs()
        p = torch.softmax(ld, 0)
        dw = (dl + 2.0) * U                                  # __expf(l - max), relative, per frame
    else:
        p = torch.full_like(xd, 1.0 / T)
        dw = torch.zeros_like(xd)
    m = (p * xd).sum(0)
    d = xd - m
    var = (p * d * d).sum(0)
    if var_div_t1:
        var = var * T / max(T - 1, 1)
    sd = torch.sqrt(torch.clamp(var, min=1e-12))
    cu = (n + 2) * U                                         # a sum of weights, or of weighted values: the chain and the division
    e_m = cu * ((p * xd.abs()).sum(0) + m.abs()) + (p * dw * (xd.abs() + m.abs())).sum(0) + U * m.abs()
    e_d = e_m + U * d.abs()
    e_var = 2.0 * (p * d.abs() * e_d).sum(0) + e_m * e_m + 2.0 * cu * var + 2.0 * (p * dw * d * d).sum(0) + 3.0 * U * var
    # |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)), the kernel's root being at least 1e-6 behind the 1e-12 clamp
    e_sd = e_var / (sd + torch.clamp(sd - e_var / sd, min=1e-6)) + U * sd
    ref, e = torch.cat([m, sd]), torch.cat([e_m, e_sd])
    if scale is not None:
        sh = shift.double()
        if shift_low:
            sh = torch.cat([sh[:C], sh[:C]])
        ref, e = ref * scale.double() + sh, e * scale.double().abs() + U * (ref * scale.double() + sh).abs()
    return ref, ulp(ref, dtype) + e


def col_stats_inputs(T, C, dtype, seed=None, device="cpu"):
    """x with a per-channel offset and one constant channel (the 1e-12 clamp); logits whose spread is 0 in every fourth channel
    (flat weights) and grows to 6 in the others (a few frames take most of the weight)."""
    seed = 900 + T if seed is None else seed
    x = rnd(T, C, seed=seed, scale=1.5, device=device) + rnd(1, C, seed=seed + 1, device=device)
    x[:, 3] = 0.625
    spread = (torch.arange(C, dtype=torch.float64, device=device) % 4) * 2.0
    logit = rnd(T, C, seed=seed + 2, device=device) * spread
    scale = (1.0 + rnd(2 * C, seed=seed + 3, scale=0.1, device=device)).float()
    shift = rnd(2 * C, seed=seed + 4, scale=0.3, device=device).float()
    shift[C:] += 1.0                                         # shift[C + c] is nowhere near shift[c]
    return x.to(dtype), logit.to(dtype), scale, shift
