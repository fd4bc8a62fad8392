"""The NumPy restatement of the multigrid solvers, once: the level, the pair descriptor, the
one-dimensional stencils, the two transfers, the sweep, Cycle(l), the solve, the MGCG preconditioner, its set-up and the
replay of the recurrences -- for every grid kind, transfer, line stage and precision the case modules build problems for.

Everything follows the normative definitions of include/neptune_hip.h: arithmetic in the element type with one `.astype(dt)`
per operation (numpy never fuses), the transfer stencils along the last dimension first with kept dimensions skipped, the
operator itself from the oracle.  No reduction enters a field, so the fields of a run are fully determined and the tests
compare them bit for bit; the sums (r . r, p . q, r . z) are compared against the exact sum of the restatement's own terms
with the bound two summation orders may differ by (monitor_cases.reference_sum, cg_cases.dot_terms).

A level is a Level; it may carry `.axes`, the pair that leaves it (a Pair, or a plain tuple of dimensions: a vertex-centred
pair over them; default all dimensions), and `.stages`, a list of (axis, lo, inv, up) line stages (empty: the point sweep
with minv).  A problem is a list of levels, or for mixed precision an object with .A (the f64 outer operator), .levels (f32),
.shape and .where (mgcgmixed_cases.Problem).

The bits of the stencils are the contract: tests/golden/mg_restatement.json holds what the case modules' former own copies
of all this produced, and tests/test_mgfuzz_host.py holds this module to it."""
import math

import numpy as np

import cg_cases as cgc
import helpers
import monitor_cases as mc

D, S = np.float64, np.float32
RSCALE = 4.0
EVEN, ODD = 0, 1            # NEPTUNE_HIP_MG_RIM_EVEN / _ODD
RULE = {"neumann": EVEN, "dirichlet": ODD}
FACE = {EVEN: "neumann", ODD: "dirichlet"}


# ================================================================ the level and its operators
class Operator:
    """the oracle's A for one module text (and its fixed inputs): q = A(u) into a fresh array"""

    def __init__(self, text, *rest):
        self.module = helpers.oracle.Module.parse(text)
        self.rest = rest

    def __call__(self, u: np.ndarray) -> np.ndarray:
        out = np.zeros_like(u)
        self.module.call("entry", out, u, *self.rest)
        return out


class OmegaOperator:
    """the oracle's A for one module text, on Omega: q = A(u) on `where`, +0 on every other cell.  That is what q holds where
    the solvers read it outside Omega: the MGCG drivers stream q over the whole box, a launch writes Omega (and copies p = +0
    through between the launch region and the module's bounds), and where the region is not the whole box the drivers
    zero-fill q once.  Sweeps, stages and transfers read q on Omega only."""
    _parsed = {}

    def __init__(self, text, where):
        if text not in self._parsed:
            self._parsed[text] = Operator(text)
        self.A, self.where, self.rest = self._parsed[text], tuple(where), ()

    def __call__(self, u):
        out = np.zeros_like(u)
        out[self.where] = self.A(u)[self.where]
        return out


class Level:
    """one level of the restatement: A (a callable), Omega as a tuple of slices, minv, rscale; x, b, q are its fields"""

    def __init__(self, A, shape, where, minv, dtype, rscale=RSCALE):
        self.A, self.shape, self.where, self.minv, self.rscale = A, tuple(shape), tuple(where), minv, rscale
        self.dt = np.dtype(dtype).type
        self.m = tuple(s.stop - s.start for s in self.where)
        self.x = self.b = self.q = None


# ================================================================ the pair that leaves a level
class Pair(tuple):
    """the dimensions transferred between a level and the next one (the tuple itself), and how: .kind = "coarsened"
    (vertex-centred, m_fine = 2 m_coarse + 1, full weighting and linear interpolation: the only transfers it has) or "halved"
    (cell-centred, m_fine = 2 m_coarse); of a halved pair .prolong = "constant" | "linear", .restrict = "average" | "linear"
    and .rim[d] = (low, high) rule of field dimension d, EVEN or ODD, the one array that serves both linear transfers"""

    def __new__(cls, axes, kind="coarsened", rim=None, prolong="constant", restrict="average"):
        self = super().__new__(cls, axes)
        assert kind in ("coarsened", "halved") and prolong in ("constant", "linear") and restrict in ("average", "linear")
        assert kind == "halved" or (rim is None and prolong == "constant" and restrict == "average")
        self.kind, self.prolong, self.restrict = kind, prolong, restrict
        self.rim = None if rim is None else tuple((int(lo), int(hi)) for lo, hi in rim)
        assert self.rim is None or all(v in (EVEN, ODD) for pair in self.rim for v in pair)
        assert self.rim is not None or (prolong, restrict) == ("constant", "average")
        return self

    @property
    def halved(self):
        return self.kind == "halved"

    @property
    def symmetric(self):
        """whether the restriction is the prolongation's transpose (up to the factor): what MGCG needs"""
        return (self.prolong == "linear") == (self.restrict == "linear")


def Halved(axes):
    """a cell-centred pair with the averaging restriction and the constant prolongation"""
    return Pair(axes, "halved")


def Linear(axes, rim):
    """a cell-centred pair prolonged linearly (the restriction stays the averaging one)"""
    return Pair(axes, "halved", rim, prolong="linear")


def Transfers(axes, rim, prolong="linear", restrict="linear"):
    """a cell-centred pair, both transfers chosen"""
    return Pair(axes, "halved", rim, prolong, restrict)


def pair_of(axes, rank):
    """a Pair as it is; a plain tuple of dimensions (None: all of them) as the vertex-centred pair over them"""
    return axes if isinstance(axes, Pair) else Pair(range(rank) if axes is None else axes)


def axes_of(L):
    """the pair that leaves level L: L.axes, default every dimension vertex-centred"""
    return pair_of(getattr(L, "axes", None), len(L.shape))


def transfer_of(axes, rank):
    """(prolong kind, restrict kind, low rules, high rules) of a level's .axes as neptune_hip_mg_transfer_t holds them"""
    pair = pair_of(axes, rank)
    rim = pair.rim or ((EVEN, EVEN),) * rank
    return (int(pair.prolong == "linear"), int(pair.restrict == "linear"), [lo for lo, _ in rim], [hi for _, hi in rim])


def faces_of(rim):
    """the Python layer's faces= for a rule array"""
    return [(FACE[lo], FACE[hi]) for lo, hi in rim]


def rim_of(faces, rank):
    """((low, high) rule per dimension) for faces = "neumann" / "dirichlet" or a (low, high) pair of them per dimension"""
    if isinstance(faces, str):
        faces = [(faces, faces)] * rank
    assert len(faces) == rank
    return tuple((RULE[lo], RULE[hi]) for lo, hi in faces)


def complement(rim):
    return tuple((1 - lo, 1 - hi) for lo, hi in rim)


# ================================================================ the one-dimensional stencils
def _weigh(d, axis):
    """t = ((0.25 a-) + (0.5 a0)) + (0.25 a+) along `axis`, centred on the odd interior indices"""
    dt = d.dtype.type
    n = d.shape[axis]
    take = lambda start: np.take(d, np.arange(start, n - 2 + start, 2), axis=axis)
    with np.errstate(invalid="ignore", over="ignore"):
        qm = (dt(0.25) * take(0)).astype(dt)
        h0 = (dt(0.5) * take(1)).astype(dt)
        qp = (dt(0.25) * take(2)).astype(dt)
        s = (qm + h0).astype(dt)
        return (s + qp).astype(dt)


def _interp(e, axis):
    """one-dimensional interpolation along `axis`: m -> 2 m + 1 cells; odd i takes e[(i - 1) / 2], even i takes
    0.5 * (e[i / 2 - 1] + e[i / 2]) with e[-1] = e[m] = +0"""
    dt = e.dtype.type
    m = e.shape[axis]
    pad = [(0, 0)] * e.ndim
    pad[axis] = (1, 1)
    p = np.pad(e, pad, constant_values=dt(0))
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.take(p, np.arange(0, m + 1), axis=axis) + np.take(p, np.arange(1, m + 2), axis=axis)).astype(dt)
        h = (dt(0.5) * s).astype(dt)
    shape = list(e.shape)
    shape[axis] = 2 * m + 1
    out = np.empty(shape, e.dtype)
    even = [slice(None)] * e.ndim
    even[axis] = slice(0, None, 2)
    odd = [slice(None)] * e.ndim
    odd[axis] = slice(1, None, 2)
    out[tuple(even)] = h
    out[tuple(odd)] = e
    return out


def _mean(d, axis):
    """t = 0.5 * (a[2 j] + a[2 j + 1]) along `axis`: one rounded addition and the exact scaling"""
    dt = d.dtype.type
    n = d.shape[axis]
    assert n % 2 == 0
    take = lambda start: np.take(d, np.arange(start, n, 2), axis=axis)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (take(0) + take(1)).astype(dt)
        return (dt(0.5) * s).astype(dt)


def _repeat(e, axis):
    """m -> 2 m cells along `axis`: fine cell i takes e[i / 2] itself (no operation)"""
    return np.repeat(e, 2, axis=axis)


def _linear(e, axis, rule_lo, rule_hi):
    """m -> 2 m cells along `axis`: fine 2 j takes 0.75 e[j] + 0.25 e[j - 1], fine 2 j + 1 takes 0.75 e[j] + 0.25 e[j + 1], e
    padded with + (EVEN) or - (ODD) its own edge"""
    dt = e.dtype.type
    m = e.shape[axis]
    take = lambda a, idx: np.take(a, idx, axis=axis)
    first, last = take(e, [0]), take(e, [m - 1])
    with np.errstate(invalid="ignore", over="ignore"):
        padded = np.concatenate([-first if rule_lo == ODD else first, e, -last if rule_hi == ODD else last], axis=axis)
        p = (dt(0.75) * e).astype(dt)
        sm = (dt(0.25) * take(padded, np.arange(0, m))).astype(dt)
        sp = (dt(0.25) * take(padded, np.arange(2, m + 2))).astype(dt)
        even = (p + sm).astype(dt)
        odd = (p + sp).astype(dt)
    shape = list(e.shape)
    shape[axis] = 2 * m
    out = np.empty(shape, e.dtype)
    sl = [slice(None)] * e.ndim
    sl[axis] = slice(0, None, 2)
    out[tuple(sl)] = even
    sl[axis] = slice(1, None, 2)
    out[tuple(sl)] = odd
    return out


def _gather(a, axis, rule_lo, rule_hi):
    """2 m -> m cells along `axis`: the four operands a[2 j - 1 .. 2 j + 2] with the weights 1/4, 3/4, 3/4, 1/4, a padded with
    + (EVEN) or - (ODD) its own edge: the FINE intermediate array padded, exactly the transpose of padding the coarse one in
    _linear"""
    dt = a.dtype.type
    n = a.shape[axis]
    assert n % 2 == 0 and n >= 2
    m = n // 2
    take = lambda arr, idx: np.take(arr, idx, axis=axis)
    first, last = take(a, [0]), take(a, [n - 1])
    with np.errstate(invalid="ignore", over="ignore"):
        padded = np.concatenate([-first if rule_lo == ODD else first, a, -last if rule_hi == ODD else last], axis=axis)
        j = np.arange(m)
        sm = (dt(0.25) * take(padded, 2 * j)).astype(dt)            # a[2 j - 1]
        p0 = (dt(0.75) * take(padded, 2 * j + 1)).astype(dt)        # a[2 j]
        p1 = (dt(0.75) * take(padded, 2 * j + 2)).astype(dt)        # a[2 j + 1]
        sp = (dt(0.25) * take(padded, 2 * j + 3)).astype(dt)        # a[2 j + 2]
        u = (sm + p0).astype(dt)
        v = (p1 + sp).astype(dt)
        w = (u + v).astype(dt)
        return (dt(0.5) * w).astype(dt)


# ================================================================ the two transfers
def _along(a, pair, stencil):
    """`stencil(a, axis)` along every dimension of the pair: the last dimension first, kept dimensions skipped"""
    for axis in reversed(range(a.ndim)):
        if axis in pair:
            a = stencil(a, axis)
    return a


def restrict(b_f, q_f, where_f, rscale, b_c, x_c, where_c, axes=None):
    """-> new (b_c, x_c): b_c = rscale * R(b_f - q_f) and x_c = +0 on the coarse Omega, R along the pair `axes`: full weighting
    (coarsened), the mean or the transposed linear prolongation P^T / 2 by the rules .rim (halved); every other cell keeps its
    bits; nothing outside where_f is read"""
    dt = b_f.dtype.type
    pair = pair_of(axes, b_f.ndim)
    if not pair.halved:
        stencil = _weigh
    elif pair.restrict == "linear":
        stencil = lambda t, axis: _gather(t, axis, *pair.rim[axis])
    else:
        stencil = _mean
    with np.errstate(invalid="ignore", over="ignore"):
        t = _along((b_f[where_f] - q_f[where_f]).astype(dt), pair, stencil)
        bc, xc = b_c.copy(), x_c.copy()
        bc[where_c] = (dt(rscale) * t).astype(dt)
    xc[where_c] = dt(0)
    return bc, xc


def prolong_add(x_c, where_c, x_f, where_f, axes=None):
    """-> a new x_f: x_f + P(x_c) on the fine Omega, P along the pair `axes`: linear interpolation (coarsened), the coarse
    cell's value itself or the linear prolongation by the rules .rim (halved); every other cell keeps its bits; nothing
    outside where_c is read"""
    dt = x_f.dtype.type
    pair = pair_of(axes, x_f.ndim)
    if not pair.halved:
        stencil = _interp
    elif pair.prolong == "linear":
        stencil = lambda e, axis: _linear(e, axis, *pair.rim[axis])
    else:
        stencil = _repeat
    e = _along(x_c[where_c], pair, stencil)
    out = x_f.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[where_f] = (x_f[where_f] + e).astype(dt)
    return out


# ================================================================ the smoothers
def smooth(q, b, minv, x, where):
    """on Omega: d = b - q, w = minv * d, x = x + w; -> a new x, every other cell keeps its bits"""
    dt = x.dtype.type
    out = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b[where] - q[where]).astype(dt)
        w = (minv[where] * d).astype(dt)
        out[where] = (x[where] + w).astype(dt)
    return out


def line_stage(q, b, lo, inv, up, x, where, axis):
    """one stage from q = A(x): -> a new x; every cell outside Omega keeps its bits.  lo at i = 0, up at i = m - 1 and
    everything outside Omega are not read.  The recurrences are marched cell by cell along the line (vectorised across the
    lines only, which changes no value)."""
    dt = x.dtype.type
    view = lambda f: np.moveaxis(f[where], axis, 0)
    qv, bv, lv, iv, uv, xv = view(q), view(b), view(lo), view(inv), view(up), view(x)
    m = xv.shape[0]
    g = [None] * m
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(m):
            d = (bv[i] - qv[i]).astype(dt)
            if i == 0:
                g[0] = (d * iv[0]).astype(dt)
            else:
                t = (lv[i] * g[i - 1]).astype(dt)
                s = (d - t).astype(dt)
                g[i] = (s * iv[i]).astype(dt)
        new = np.empty(xv.shape, x.dtype)
        e = g[m - 1]
        new[m - 1] = (xv[m - 1] + e).astype(dt)
        for i in range(m - 2, -1, -1):
            t = (uv[i] * e).astype(dt)
            e = (g[i] - t).astype(dt)
            new[i] = (xv[i] + e).astype(dt)
    out = x.copy()
    out[where] = np.moveaxis(new, 0, axis)
    return out


def first_stage(b, lo, inv, up, x, where, axis):
    """the stage on q = +0, x = +0 without reading either: d_i = b_i, the recurrences of the plain stage, x_i = (+0) + e_i.
    -> a new x: Omega from b alone (x on Omega is not read), every cell outside Omega keeps its bits"""
    dt = x.dtype.type
    view = lambda f: np.moveaxis(f[where], axis, 0)
    bv, lv, iv, uv = view(b), view(lo), view(inv), view(up)
    m = bv.shape[0]
    g = [None] * m
    zero = np.zeros(bv.shape[1:], x.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(m):
            d = bv[i]
            if i == 0:
                g[0] = (d * iv[0]).astype(dt)
            else:
                t = (lv[i] * g[i - 1]).astype(dt)
                s = (d - t).astype(dt)
                g[i] = (s * iv[i]).astype(dt)
        new = np.empty(bv.shape, x.dtype)
        e = g[m - 1]
        new[m - 1] = (zero + e).astype(dt)
        for i in range(m - 2, -1, -1):
            t = (uv[i] * e).astype(dt)
            e = (g[i] - t).astype(dt)
            new[i] = (zero + e).astype(dt)
    out = x.copy()
    out[where] = np.moveaxis(new, 0, axis)
    return out


def first_sweep(levels, r):
    """the cycle's first pre-sweep on a level 0 without stages, from z = 0 with A(0) = 0: z = minv_0 * r on every cell, one
    rounding (minv_0 is +0 outside Omega)"""
    L0 = levels[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return (L0.minv * r).astype(L0.dt)


# ---------------------------------------------------------------- the mixed form's kernels (f64 outside, f32 levels)
def narrow(a: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return a.astype(S)


def widen(a: np.ndarray) -> np.ndarray:
    return a.astype(D)


def wide_dot_terms(a32: np.ndarray, b32: np.ndarray, where):
    """-> (sum, bound) of the terms widen(a32) * widen(b32) over `where`: each term exact in f64, summed exactly; bound =
    2 (n - 1) eps64 sum |t_i|"""
    assert a32.dtype == S and b32.dtype == S
    return cgc.dot_terms(widen(a32), widen(b32), where)


def store_residual(P, x0, b0):
    """steps 1 and 2 of the mixed set-up: -> (x, r, r32, z32, rr0 as (terms' sum, bound)); what a call that runs no iteration
    leaves behind"""
    L0 = P.levels[0]
    start(P.levels)
    x = x0.copy()
    q = P.A(x)
    r = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r[P.where] = (b0[P.where] - q[P.where]).astype(D)
    rr0 = cgc.dot_terms(r, r, P.where)
    r32 = narrow(r)
    z32 = np.zeros(P.shape, S)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        z32[P.where] = (L0.minv[P.where] * r32[P.where]).astype(S)
    return x, r, r32, z32, rr0


def update(P, alpha, x, r, p, q):
    """step 2 of the mixed iteration on all cells: -> (x, r, r32, z32 after the first pre-sweep)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        x = (x + (alpha * p).astype(D)).astype(D)
        r = (r - (alpha * q).astype(D)).astype(D)
        r32 = narrow(r)
        z32 = (P.levels[0].minv * r32).astype(S)
    return x, r, r32, z32


# ================================================================ the control flow of include/neptune_hip.h
def sweep(L, reverse=False):
    """a level without stages: q = A(x), then the point smoother; with k stages: all k, each after its own apply, in order
    0 .. k-1, or k-1 .. 0 (reverse: a post-sweep)"""
    stages = getattr(L, "stages", [])
    if not stages:
        L.q = L.A(L.x)
        L.x = smooth(L.q, L.b, L.minv, L.x, L.where)
        return
    for axis, lo, inv, up in (reversed(stages) if reverse else stages):
        L.q = L.A(L.x)
        L.x = line_stage(L.q, L.b, lo, inv, up, L.x, L.where, axis)


def descend(levels, l, pre, post, coarse_sweeps):
    """q = A(x) and the restriction; Cycle(l + 1); prolongation and correction"""
    L, nxt = levels[l], levels[l + 1]
    L.q = L.A(L.x)
    nxt.b, nxt.x = restrict(L.b, L.q, L.where, L.rscale, nxt.b, nxt.x, nxt.where, axes_of(L))
    cycle(levels, l + 1, pre, post, coarse_sweeps)
    L.x = prolong_add(nxt.x, nxt.where, L.x, L.where, axes_of(L))


def cycle(levels, l, pre, post, coarse_sweeps):
    """Cycle(l)"""
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(coarse_sweeps):
            sweep(L)
        return
    for _ in range(pre):
        sweep(L)
    descend(levels, l, pre, post, coarse_sweeps)
    for _ in range(post):
        sweep(L, reverse=True)


def start(levels, x0=None, b0=None, work_fill=np.nan):
    """the state before the first cycle: the coarser x zero-filled (whole box), the coarser b and every q holding `work_fill`
    (what the device's work fields hold before the call).  With x0 and b0 (a solve) level 0 holds copies of the caller's x
    and b; without (MGCG) level 0's x and b are set per application of M."""
    for l, L in enumerate(levels):
        if l > 0:
            L.x = np.zeros(L.shape, L.dt)
            L.b = np.full(L.shape, work_fill, L.dt)
        elif x0 is not None:
            L.x, L.b = x0.copy(), b0.copy()
        L.q = np.full(L.shape, work_fill, L.dt)


def residual(L):
    """-> (rr as the exact sum of the terms (b - A(x))^2 over Omega, the bound two summation orders may differ by); L.q = A(x)"""
    L.q = L.A(L.x)
    return mc.reference_sum(L.b, L.q, L.where)


def run(levels, x0, b0, cycles, pre=2, post=2, coarse_sweeps=8, check_every=1):
    """`cycles` cycles of the solve's schedule with no tolerance: -> (rr0, [rr after each block]) as (sum, bound) pairs;
    the fields are left in `levels`"""
    start(levels, x0, b0)
    rr0 = residual(levels[0])
    checks, done = [], 0
    while done < cycles:
        for _ in range(min(check_every, cycles - done)):
            cycle(levels, 0, pre, post, coarse_sweeps)
            done += 1
        checks.append(residual(levels[0]))
    return rr0, checks


def rr_sequence(levels, x0, b0, cycles, pre=2, post=2, coarse_sweeps=8, stop_at=None):
    """[rr_0, rr after cycle 1, ...] as floats (the terms' exact sums); stop_at: a factor -- end early once
    rr <= stop_at * rr_0"""
    start(levels, x0, b0)
    seq = [residual(levels[0])[0]]
    for _ in range(cycles):
        if stop_at is not None and seq[-1] <= stop_at * seq[0]:
            break
        cycle(levels, 0, pre, post, coarse_sweeps)
        seq.append(residual(levels[0])[0])
    return seq


expected_stop = cgc.expected_stop       # what the loop's definition gives on an r . r sequence: (cycles or iterations done, checks)


def tol_between(seq, a, b):
    """a threshold at the geometric mean of seq[a] and seq[b], which must differ by at least a factor of 4: two summation
    orders move r . r by parts in 1e-13 (f64) / 1e-4 (f32), so the stop cannot hinge on rounding"""
    assert seq[b] * 4.0 <= seq[a], "precondition: consecutive check values differ by at least a factor of 4"
    return math.sqrt(seq[a] * seq[b])


# ---------------------------------------------------------------- the MGCG preconditioner
def first_pre_sweep(levels, r):
    """level 0's first pre-sweep on (x, b) = (z, r) from z = 0: with stages, stage 0 apply-free and the others plain; without,
    z = minv_0 * r on every cell"""
    L0 = levels[0]
    stages = getattr(L0, "stages", [])
    L0.b = r
    if not stages:
        L0.x = first_sweep(levels, r)
        return
    axis, lo, inv, up = stages[0]
    L0.x = first_stage(r, lo, inv, up, np.zeros(L0.shape, L0.dt), L0.where, axis)
    for axis, lo, inv, up in stages[1:]:
        L0.q = L0.A(L0.x)
        L0.x = line_stage(L0.q, L0.b, lo, inv, up, L0.x, L0.where, axis)


def rest_of_cycle(levels, sweeps, coarse_sweeps):
    """"the rest of M": everything of the cycle on level 0's (x, b) = (z, r) after its first pre-sweep -- the other pre-sweeps,
    the coarser levels, the post-sweeps, the last of which also yields r . z on the device; -> z"""
    L0 = levels[0]
    for _ in range(sweeps - 1):
        sweep(L0)
    descend(levels, 0, sweeps, sweeps, coarse_sweeps)
    for _ in range(sweeps):
        sweep(L0, reverse=True)
    return L0.x


def precondition(levels, r, sweeps=2, coarse_sweeps=8):
    """z = M(r): one V(sweeps, sweeps) cycle on A_0 z = r from z = 0 (call start(levels) once before)"""
    assert len(levels) >= 2 and sweeps >= 1
    first_pre_sweep(levels, r)
    return rest_of_cycle(levels, sweeps, coarse_sweeps)


def dense_preconditioner(levels, sweeps=2, coarse_sweeps=8):
    """M as a dense matrix over the cells of Omega_0 (C order), built column by column from unit vectors"""
    L0 = levels[0]
    n = int(np.prod(L0.m))
    M = np.empty((n, n), np.float64)
    start(levels, work_fill=0.0)
    for j in range(n):
        e = np.zeros(L0.m, L0.dt)
        e.flat[j] = 1
        r = np.zeros(L0.shape, L0.dt)
        r[L0.where] = e
        M[:, j] = precondition(levels, r, sweeps, coarse_sweeps)[L0.where].ravel()
    return M


# ---------------------------------------------------------------- MGCG: the set-up and the recurrences
class State:
    """the fields of an MGCG run: x, r, p, z (mixed: x, r, p in f64 and r32, z32); after replay also .rz0_used and .rr_own,
    numpy's own sum of r . r after the set-up"""


def is_mixed(problem):
    return hasattr(problem, "levels")


def setup(problem, x0, b0, sweeps=2, coarse_sweeps=8):
    """the definition's set-up for a list of levels or a mixed problem: -> (State, rr0, rz0), the two sums as (terms' sum,
    bound)"""
    st = State()
    if is_mixed(problem):
        st.x, st.r, st.r32, z32, rr0 = store_residual(problem, x0, b0)
        L0 = problem.levels[0]
        assert not getattr(L0, "stages", [])
        L0.x, L0.b = z32, st.r32
        st.z32 = rest_of_cycle(problem.levels, sweeps, coarse_sweeps)
        st.p = widen(st.z32)
        return st, rr0, wide_dot_terms(st.r32, st.z32, problem.where)
    L0 = problem[0]
    start(problem)
    st.x = x0.copy()
    q = L0.A(st.x)
    st.r = np.zeros_like(st.x)
    with np.errstate(invalid="ignore", over="ignore"):
        st.r[L0.where] = (b0[L0.where] - q[L0.where]).astype(L0.dt)
    rr0 = cgc.dot_terms(st.r, st.r, L0.where)
    st.z = precondition(problem, st.r, sweeps, coarse_sweeps)
    st.p = st.z.copy()
    return st, rr0, cgc.dot_terms(st.r, st.z, L0.where)


def _own(terms):
    """numpy's own sum of the terms in their element type"""
    return terms.dtype.type(np.sum(terms, dtype=terms.dtype))


def replay(problem, x0, b0, rz0=None, trace=None, sweeps=2, coarse_sweeps=8, iters=None, stop_at=None):
    """The definition's recurrences on the preconditioner above, driven by the DEVICE's scalars: iteration k takes
    alpha_k = rz_k / pq_k and beta_k = rz_(k+1) / rz_k from rz0 and the trace rows (pq_k, rz_(k+1), rr_(k+1)), each one division
    in the (outer) element type, and q from the oracle's operator -- or, with trace = None, driven by numpy's own sums for
    `iters` iterations, ending early once its own r . r <= stop_at.
    -> (State, checks, rr0, rz0_ref, scalars): checks[k] = the (terms' sum, bound) pairs of pq, rz' and rr' of the replay's own
    fields (none without a trace: there is no device sum to hold against them), rr0 / rz0_ref those of the set-up; scalars[k] = (pq, rz', numpy's own rr', broken) as used; the levels' x_l, b_l are
    left in the levels (level 0's are z and r)."""
    mixed = is_mixed(problem)
    A = problem.A if mixed else problem[0].A
    where = problem.where if mixed else problem[0].where
    dt = D if mixed else problem[0].dt
    st, rr0, rz0_ref = setup(problem, x0, b0, sweeps, coarse_sweeps)
    zr = (lambda: (widen(st.r32[where]) * widen(st.z32[where]))) if mixed else (lambda: (st.r[where] * st.z[where]).astype(dt))
    rz = dt(rz0) if trace is not None else _own(zr())
    st.rz0_used = rz
    st.rr_own = rr = _own((st.r * st.r).astype(dt))
    checks, scalars = [], []
    everywhere = tuple(slice(None) for _ in st.x.shape)
    for k in range(len(trace) if trace is not None else iters):
        if stop_at is not None and rr <= stop_at:
            break
        q = A(st.p)
        pq_ref = cgc.dot_terms(q, st.p, where) if trace is not None else None
        pq = dt(trace[k][0]) if trace is not None else _own((q[where] * st.p[where]).astype(dt))
        broken = rz == 0 or pq == 0
        alpha = dt(0) if broken else dt(rz / pq)
        if mixed:
            st.x, st.r, st.r32, z32 = update(problem, alpha, st.x, st.r, st.p, q)
            L0 = problem.levels[0]
            L0.x, L0.b = z32, st.r32
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                st.x = (st.x + (alpha * st.p).astype(dt)).astype(dt)
                st.r = (st.r - (alpha * q).astype(dt)).astype(dt)
        if mixed:
            st.z32 = rest_of_cycle(problem.levels, sweeps, coarse_sweeps)
        else:
            st.z = precondition(problem, st.r, sweeps, coarse_sweeps)
        if trace is not None:
            rz_ref = wide_dot_terms(st.r32, st.z32, where) if mixed else cgc.dot_terms(st.r, st.z, where)
            checks.append((pq_ref, rz_ref, cgc.dot_terms(st.r, st.r, everywhere)))
        rz_new = dt(trace[k][1]) if trace is not None else _own(zr())
        beta = dt(0) if broken else dt(rz_new / rz)
        with np.errstate(invalid="ignore", over="ignore"):
            st.p = ((widen(st.z32) if mixed else st.z) + (beta * st.p).astype(dt)).astype(dt)
        rr = _own((st.r * st.r).astype(dt))
        scalars.append((pq, rz_new, rr, bool(broken)))
        rz = rz_new
    return st, checks, rr0, rz0_ref, scalars


def numpy_mgcg(problem, x0, b0, iters, sweeps=2, coarse_sweeps=8, stop_at=None):
    """the recurrences with numpy's own sums: -> the r . r sequence [rr_0, rr_1, ...] (floats), for the stop tests and the
    convergence checks; stop_at: end early once r . r <= stop_at"""
    st, _, _, _, scalars = replay(problem, x0, b0, None, None, sweeps, coarse_sweeps, iters, stop_at)
    return [float(st.rr_own)] + [float(s[2]) for s in scalars]
