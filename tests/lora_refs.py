"""References of the adapter bank's shrink kernels (csrc/lora.hip: lora_shrink_kernel<T, NCH> and lora_shrink_mix_kernel<T, NCH>) for
test_lora_kernels_gpu.py and test_lora_refs_cpu.py: seeded operands, the float64 reference on the ROUNDED operands, the derived
bound, a float32 stand-in that walks the kernel's order of operations on the CPU, and the negative controls.  Nothing here calls
the library under test.

The operation.  Row m names adapters through an id (itts_lora_shrink) or a record of up to four (id, weight) entries
(itts_lora_shrink_mix).  For every entry (a, w) with 0 <= a < n:  u[m][a * rp + j] = w32 * sum_k x[m][k] A[a][j][k], w32 the fp32
value of the weight (1 in the id launch); of two entries with one id the earlier one counts; every other column of u[m][:Kx] is 0,
the rank padding (rows of A[a] at and behind the adapter's rank are zeros) included.  mag = |w32| sum_k |x| |A|.

The kernel's arithmetic, and the bound derived from it.  E = elements of a 16-byte piece (8 in bf16 / f16, 4 in fp32); one pass of
the workgroup's 256 lanes covers P = 256 E elements (2048 / 1024).
  * A lane owns the pieces p = tid + 256 t of the row and adds their E products one after the other into one fp32 accumulator per
    row of A: E * ceil(K / P) fma at most.  The product of two bf16 (8 x 8 significand bits) or two f16 (11 x 11) values is exact in
    fp32, so the fma is one rounded addition; in fp32 the fma rounds once by definition.  Either way: one rounding of at most
    2^-24 |partial sum| per term, and every partial sum is at most the lane's share of sum |x| |A|.
  * reduce16 adds the 64 lanes of a wave in a tree of depth 6 (four halving steps, then two more butterflies): 6 roundings on the
    path of any one term.  The four waves' partials are added in wave order: 3 more.  The weight is one fp32 multiply: 1 more.
  * So the fp32 value in front of the store is within C(K) mag of the exact one, C(K) = (E ceil(K / P) + 10) 2^-24 (first order in
    2^-24; the largest count here is 90), and the store rounds it to T once:
        bound = 0.5 ulp_T(|ref| + C(K) mag) + C(K) mag.
    The spacing is taken at |ref| + C mag, so a value the fp32 error pushes over a binade edge is covered.  A column nobody names
    has ref = mag = 0 and a bound of half the smallest subnormal: only an exact zero passes.
Nothing in the bound is fitted to what a kernel returned.

The stand-in (`lane_sums`, `standin`) reproduces that order in float32: per-lane sequential fma over the lane's pieces (the product
and the addition are done in float64 and rounded to float32 once -- the fma of the 16-bit types exactly, the fp32 one up to a double
rounding that needs the 53-bit sum to end on a float32 midpoint), the reduce16 tree lane by lane, the waves in order, the weight,
one rounding to T.  test_lora_refs_cpu.py holds it to the bound at every case of the GPU file and proves that every control below
exceeds the bound against it, with no GPU.

Negative controls: deliberately wrong references (`control`).  The bound of a control is the formula above at the wrong reference
with the true mag.  `rounded twice` is declared for the 16-bit types only: in fp32 the storage type is the accumulation type, a
rounding to T in front of the weight is one more fp32 rounding, and C(K) already grants at least 14 of those -- by the derivation
the bound cannot, and need not, tell them apart.  `stash dropped` (pieces t > 8 of the entries after a record's first read as zeros)
changes the reference only if a lane has a piece 9: K > 9 P."""
import torch

from fp64_check import rnd, tname, ulp  # noqa: F401

NWV, XT, NE = 4, 8, 4              # LORA_NWV, LORA_MIX_XT, ITTS_LORA_MIX_ENTRIES
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
RANKS = {16: (1, 9, 16), 32: (17, 24, 32), 48: (4, 16, 40), 64: (49, 56, 64)}
N = 3
M_MAX = 17


def E(dtype):
    return 4 if dtype == torch.float32 else 8


def KS(dtype):
    return 4 * E(dtype)


def P(dtype):
    return NWV * 64 * E(dtype)


def kx(n, rp):
    return (n * rp + 31) // 32 * 32


def f32(w):
    return torch.tensor(w, dtype=torch.float32).item()


def form_ks(dtype):
    """KS: one lane group works; P - KS / P / P + KS: the last lanes of the last wave lack or have a piece, one group has a second."""
    ks, p = KS(dtype), P(dtype)
    return [ks, p - ks, p, p + ks, 1280, 5120]


def stash_ks(dtype):
    """9 P: every later piece of a lane sits in the LDS stash; 9 P + KS: the first lanes fetch piece 9 again in every entry."""
    return [9 * P(dtype), 9 * P(dtype) + KS(dtype)]


FORMS = [(dtype, rp, K) for dtype in DTYPES for rp in (16, 32, 48, 64) for K in form_ks(dtype)]
STASH = [(dtype, rp, K) for dtype in DTYPES for rp in (32, 64) for K in stash_ks(dtype)]
LIMIT = [(dtype, n, rp) for dtype in (torch.bfloat16, torch.float32) for n, rp in ((8, 64), (32, 16))]     # Kx = 512, K = 1280, M = 5


def form_id(v):
    return tname(v) if isinstance(v, torch.dtype) else str(v)


# ------------------------------------------------------------------------------------------------------------ bound
def c_of(dtype, K):
    return (E(dtype) * -(-K // P(dtype)) + 10) * 2.0 ** -24


def bound(ref, mag, dtype, K):
    c = c_of(dtype, K)
    return 0.5 * ulp(ref.abs() + c * mag, dtype) + c * mag


def round_t(v, dtype):
    """float64 -> the nearest value of T's grid (ties to even), still float64."""
    u = ulp(v, dtype)
    return torch.round(v / u) * u


# ------------------------------------------------------------------------------------------------------------ operands
class Case:
    """x T [M][K] (sigma 1), the bank T [n + 2][rp][K]: adapter a of rank ranks[a] with entries of sigma 0.25 / sqrt(K), its scaling
    (a + 1) folded in at fp32, zero rows behind the rank, all rounded to T -- a dot has sigma 0.25 (a + 1), so the weight 1e4 stays
    inside f16 and 1e-4 reaches its subnormals.  The two spare adapters behind the bank's n hold sigma 3: a kernel that ignored
    the id guard would read them.  dots / mags: float64 [M][n][rp] from the rounded operands."""

    def __init__(self, dtype, K, rp, M=M_MAX, n=N):
        self.dtype, self.K, self.rp, self.M, self.n, self.Kx = dtype, K, rp, M, n, kx(n, rp)
        self.ranks = tuple(RANKS[rp][a % 3] for a in range(n))
        seed = (DTYPES.index(dtype) * 100 + rp) * 100000 + K * 3 + n
        self.x = rnd(M, K, seed=seed).to(dtype)
        A = torch.zeros(n + 2, rp, K, dtype=torch.float32)
        for a, r in enumerate(self.ranks):
            A[a, :r] = rnd(r, K, seed=seed + 1 + a, scale=0.25 / K ** 0.5).float() * float(a + 1)
        A[n:] = rnd(2, rp, K, seed=seed + 999, scale=3.0).float()
        self.bank = A.to(dtype)
        self.Ad = self.bank[:n].double()
        self.dots = self.dots_of()
        self.mags = torch.einsum("ark,mk->mar", self.Ad.abs(), self.x.double().abs())
        self._sums = None

    def dots_of(self, xd=None, keep=None):
        """[M][n][rp] float64 of another x, or of the k that `keep` (bool [K]) selects."""
        xd = self.x.double() if xd is None else xd
        if keep is not None:
            xd = xd * keep.double()
        return torch.einsum("ark,mk->mar", self.Ad, xd)

    def piece(self):
        """Of every k: the piece's pass t and its lane tid."""
        p = torch.arange(self.K) // E(self.dtype)
        return p // (NWV * 64), p % (NWV * 64)

    def sums(self):
        if self._sums is None:
            self._sums = lane_sums(self)
        return self._sums


_cases = {}


def case(dtype, K, rp, M=M_MAX, n=N):
    """The operands and references of one (dtype, K, rp), made once; only the latest few are kept (the stash cases hold 50 MB)."""
    key = (dtype, K, rp, M, n)
    if key not in _cases:
        while len(_cases) >= 3:
            _cases.pop(next(iter(_cases)))
        _cases[key] = Case(dtype, K, rp, M, n)
    return _cases[key]


# ------------------------------------------------------------------------------------------------------------ records and ids
def kinds(m, n=N):
    """Ten kinds of record, the adapters they name turning with the row: the six of test_lora_mix_kernels_gpu.py, then a zero and
    a negative weight, a large and a tiny one, ids outside the bank (n, n + 1, -7: empty entries) around a live one, and one id in
    entries 0 and 2 (entry 0 counts)."""
    a, b, c = m % n, (m + 1) % n, (m + 2) % n
    return [[], [(a, 1.0)], [(a, 0.35)], [(a, 0.7), (b, 0.3)], [(0, 0.5), (1, -0.75), (2, 1.25)], [(2, 1.25), (0, 0.5), (1, -0.75)],
            [(a, 0.0), (b, -0.6)], [(a, 1e4), (b, 1e-4)], [(n, 0.9), (a, 0.35), (n + 1, 1.1), (-7, 2.0)],
            [(a, 0.35), (b, 0.7), (a, -0.9), (c, 0.3)]]


def mix_sets(M, n=N):
    """Record sets of M rows: the kinds in rotation (every kind at M = 1, one after the other)."""
    return [[kinds(m, n)[(m + shift) % 10] for m in range(M)] for shift in (range(10) if M == 1 else (0, 1, 2))]


def stash_mix(n=N):
    """M = 3: records of 1, 2 and 4 entries (the 4-entry one repeats an id: four entries walk the row, three slots are written)."""
    return [[(0, 0.35)], [(1, 0.7), (2, -0.75)], [(1, 0.35), (2, 0.7), (1, -0.9), (0, 0.3)]]


def limit_mix(n):
    return [[(0, 0.35), (n - 1, -0.75)], [(n - 1, 1.0)], [(n // 2, 0.7), (0, 0.3), (n - 1, 1.25), (1, -0.6)], [], [(n - 1, 0.35), (n, 0.5)]]


def limit_ids(n):
    return [0, n - 1, n // 2, -1, n - 1]


ID_POOL = (-1, 0, 1, 2, N, N + 1, -7)


def id_sets(M):
    if M == 1:
        return [[v] for v in ID_POOL]
    return [[ID_POOL[(i * 3 + s) % 7] for i in range(M)] for s in (0, 1)] + [[1] * M]


def as_records(ids, place=0):
    """The records {id, 1.0} of an id launch, the entry standing at `place`."""
    return [[(-1, 0.0)] * place + [(a, 1.0)] for a in ids]


def moved(recs):
    """The same entries in the opposite order, pushed to the END of the record (empty entries in front).  A record that names one
    id twice stays as it is: there the order decides."""
    out = []
    for r in recs:
        live = [a for a, _ in r]
        out.append(r if len(set(live)) < len(live) else [(-1, 0.0)] * (NE - len(r)) + r[::-1])
    return out


def raw_records(recs):
    """uint8 [len(recs)][32]: itts_lora_mix_row as the kernel reads it, four (int32 id, float32 weight), unused entries (-1, 0).
    Built from the raw values: nothing is refused, a repeated id or an id outside the bank included."""
    ids = torch.full((len(recs), NE), -1, dtype=torch.int32)
    wts = torch.zeros(len(recs), NE, dtype=torch.float32)
    for m, r in enumerate(recs):
        assert len(r) <= NE
        for j, (a, w) in enumerate(r):
            ids[m, j], wts[m, j] = a, w
    return torch.stack([ids, wts.view(torch.int32)], -1).contiguous().view(torch.uint8).view(len(recs), 32)


# ------------------------------------------------------------------------------------------------------------ reference
def expected(c, recs, rows, dots=None, later=None, twice=False):
    """ref, mag float64 [len(recs)][Kx] and `zero` (bool: the columns that must be exactly 0 -- unnamed slots, the Kx padding and
    the rank padding of the named ones) for the records `recs` over the case's rows `rows`.  dots: the record's first live entry
    is computed from these (default: the case's own), the entries behind it from `later` (default: dots).  twice: the control
    round_T(w round_T(dot))."""
    dots = c.dots if dots is None else dots
    later = dots if later is None else later
    ref = torch.zeros(len(recs), c.Kx, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    zero = torch.ones(len(recs), c.Kx, dtype=torch.bool)
    for i, (m, rec) in enumerate(zip(rows, recs)):
        live = [(a, w) for a, w in rec if 0 <= a < c.n]
        for pos in range(len(live) - 1, -1, -1):          # backwards: of two entries with one id the earlier is written last
            a, w = live[pos]
            w32 = f32(w)
            d = (dots if pos == 0 else later)[m, a]
            own = slice(a * c.rp, (a + 1) * c.rp)
            ref[i, own] = round_t(w32 * round_t(d, c.dtype), c.dtype) if twice else w32 * d
            mag[i, own] = abs(w32) * c.mags[m, a]
            zero[i, own] = torch.arange(c.rp) >= c.ranks[a]
    return ref, mag, zero


GENERAL = ("wave 3 left out", "last piece left out", "adapter a+1 in slot a", "x of row m+1", "rank padding filled")
MIX_ONLY = ("weights swapped", "weight ignored", "rounded twice")


def controls_for(dtype, K, M, mix):
    """The controls declared for a launch.  They run where every wave has pieces and a lane has more than one (P + KS), and at the
    two stash boundaries, on the launches of at least three rows."""
    p, ks = P(dtype), KS(dtype)
    if K not in (p + ks, 9 * p, 9 * p + ks) or M < 3:
        return ()
    out = GENERAL
    if mix:
        out += tuple(n for n in MIX_ONLY if n != "rounded twice" or dtype != torch.float32)
        if K >= 9 * p:
            out += ("stash shifted",)
        if K > 9 * p:
            out += ("stash dropped",)
    return out


def control(c, name, recs, rows):
    """The wrong reference `name` of `expected(c, recs, rows)`."""
    t, tid = c.piece()
    if name == "wave 3 left out":
        return expected(c, recs, rows, dots=c.dots_of(keep=tid // 64 != 3))[0]
    if name == "last piece left out":
        return expected(c, recs, rows, dots=c.dots_of(keep=torch.arange(c.K) < c.K - E(c.dtype)))[0]
    if name == "adapter a+1 in slot a":
        return expected(c, recs, rows, dots=c.dots.roll(-1, 1))[0]
    if name == "x of row m+1":
        return expected(c, recs, rows, dots=c.dots.roll(-1, 0))[0]
    if name == "rank padding filled":
        pad = torch.stack([torch.arange(c.rp) >= r for r in c.ranks])[None]
        return expected(c, recs, rows, dots=torch.where(pad, c.dots.roll(-1, 1), c.dots))[0]
    if name == "weights swapped":
        out = []
        for r in recs:
            live = [j for j, (a, _) in enumerate(r) if 0 <= a < c.n]
            r = list(r)
            if len(live) >= 2:
                i, j = live[0], live[1]
                r[i], r[j] = (r[i][0], r[j][1]), (r[j][0], r[i][1])
            out.append(r)
        return expected(c, out, rows)[0]
    if name == "weight ignored":
        return expected(c, [[(a, 1.0) for a, _ in r] for r in recs], rows)[0]
    if name == "rounded twice":
        return expected(c, recs, rows, twice=True)[0]
    if name == "stash shifted":            # entries after the first: piece t = 1 .. 8 of a lane taken from its piece t - 1
        xd = c.x.double()
        p = P(c.dtype)
        src = torch.arange(c.K)
        src = torch.where((t >= 1) & (t <= XT), src - p, src)
        return expected(c, recs, rows, later=c.dots_of(xd=xd[:, src]))[0]
    if name == "stash dropped":            # entries after the first: pieces t > 8 read as zeros
        return expected(c, recs, rows, later=c.dots_of(keep=t <= XT))[0]
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------ stand-in
def _half(v, half, off):
    """reduce_half<HALF, OFF> over v [..., 2 * half, 64]: a lane keeps the half its bit OFF selects and adds its partner's."""
    lane = torch.arange(64)
    other = v[..., lane ^ off]
    lo = v[..., :half, :] + other[..., :half, :]
    hi = v[..., half:, :] + other[..., half:, :]
    return torch.where((lane & off) != 0, hi, lo)


def reduce16(v):
    """v float32 [..., 16, 64] (accumulator, lane) -> [..., 16]: the wave's sum of every accumulator in reduce16's order, read from
    the lane that stores it (lane = 4 j)."""
    lane = torch.arange(64)
    for half, off in ((8, 32), (4, 16), (2, 8), (1, 4)):
        v = _half(v, half, off)
    s = v[..., 0, :]
    s = s + s[..., lane ^ 2]
    s = s + s[..., lane ^ 1]
    return s[..., ::4]


def lane_sums(c):
    """float32 [M][n][rp]: what the kernel holds in front of the weight -- per lane the sequential fma over its pieces, reduce16
    per 16-row chunk, the four waves in order."""
    e, p = E(c.dtype), P(c.dtype)
    T = -(-c.K // p)
    pad = T * p - c.K                    # pieces no lane has: x = A = 0 leaves an accumulator as it is
    x = torch.nn.functional.pad(c.x.double(), (0, pad)).view(c.M, 1, 1, T, NWV * 64, e)
    A = torch.nn.functional.pad(c.bank[:c.n].double(), (0, pad)).view(1, c.n, c.rp, T, NWV * 64, e)
    acc = torch.zeros(c.M, c.n, c.rp, NWV * 64, dtype=torch.float32)
    for t in range(T):
        for i in range(e):
            acc = (x[..., t, :, i] * A[..., t, :, i] + acc.double()).float()
    v = acc.view(c.M, c.n, c.rp // 16, 16, NWV, 64).permute(0, 1, 2, 4, 3, 5)       # [M][n][chunk][wave][16][lane]
    part = reduce16(v)                                                              # [M][n][chunk][wave][16]
    s = part[..., 0, :]
    for w in range(1, NWV):
        s = s + part[..., w, :]
    return s.reshape(c.M, c.n, c.rp)


def standin(c, recs, rows):
    """T [len(recs)][Kx]: the kernel's output for the records, from lane_sums, the fp32 weight and one rounding to T."""
    s = c.sums()
    y = torch.zeros(len(recs), c.Kx, dtype=c.dtype)
    for i, (m, rec) in enumerate(zip(rows, recs)):
        for a, w in reversed([(a, w) for a, w in rec if 0 <= a < c.n]):
            y[i, a * c.rp:(a + 1) * c.rp] = (s[m, a] * torch.tensor(w, dtype=torch.float32)).to(c.dtype)
    return y


# ------------------------------------------------------------------------------------------------------------ the check
def verify(what, c, recs, rows, y, ok, bad, mix):
    """y T [len(recs)][Kx] (a kernel's or the stand-in's) against the reference: exact zeros where nobody writes a value, `ok` under
    the bound, and every control declared for the launch through `bad`."""
    ref, mag, zero = expected(c, recs, rows)
    yd = y.double().cpu()
    assert (yd[zero] == 0).all(), f"{what}: a column outside the named ranks is not 0"
    assert (yd[~zero] != 0).any() or not (~zero).any(), f"{what}: nothing was written"
    ok(what, yd, ref, bound(ref, mag, c.dtype, c.K))
    for name in controls_for(c.dtype, c.K, len(set(rows)), mix):
        wrong = control(c, name, recs, rows)
        bad(what, name, yd, wrong, bound(wrong, mag, c.dtype, c.K))
