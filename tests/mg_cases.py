"""Operators and the NumPy restatement of the multigrid tests.

The operator is the star of monitor_cases.star_module with centre weight 2 * rank and side weight -1 -- the unscaled Poisson
operator, one module per level shape --, rscale = 4, and damped-Jacobi weights minv = omega / (2 * rank) on Omega.

Everything here follows the normative definition of neptune_hip_mg_solve (include/neptune_hip.h): arithmetic in the element
type with one `.astype(dt)` per operation, the transfer stencils along the last dimension first, the operator itself from
the oracle.  No reduction enters a field, so the fields of a run are fully determined and the tests compare them bit for
bit; r . r is compared against the exact sum of the restatement's own terms (monitor_cases.reference_sum)."""
import math

import numpy as np

import helpers
import monitor_cases as mc

RSCALE = 4.0


def mg_module(shape, dtype=np.float64):
    """NeptuneIR text of @entry(out, in): out = 2 rank * in - (sum of the star neighbours) one cell in from every face"""
    return mc.star_module(shape, dtype, centre=float(2 * len(shape)), side=-1.0)


class Operator:
    """the oracle's A for one module text (and its fixed inputs): q = A(u) into a fresh array"""

    def __init__(self, text, *rest):
        self.module = helpers.oracle.Module.parse(text)
        self.rest = rest

    def __call__(self, u: np.ndarray) -> np.ndarray:
        out = np.zeros_like(u)
        self.module.call("entry", out, u, *self.rest)
        return out


class Level:
    """one level of the restatement: A (a callable), Omega as a tuple of slices, minv, rscale; x, b, q are its fields"""

    def __init__(self, A, shape, where, minv, dtype, rscale=RSCALE):
        self.A, self.shape, self.where, self.minv, self.rscale = A, tuple(shape), tuple(where), minv, rscale
        self.dt = np.dtype(dtype).type
        self.m = tuple(s.stop - s.start for s in self.where)
        self.x = self.b = self.q = None


# ---------------------------------------------------------------- the three kernels
def smooth(q, b, minv, x, where):
    """on Omega: d = b - q, w = minv * d, x = x + w; -> a new x, every other cell keeps its bits"""
    dt = x.dtype.type
    out = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b[where] - q[where]).astype(dt)
        w = (minv[where] * d).astype(dt)
        out[where] = (x[where] + w).astype(dt)
    return out


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


def restrict(b_f, q_f, where_f, rscale, b_c, x_c, where_c):
    """-> new (b_c, x_c): b_c = rscale * R(b_f - q_f) and x_c = +0 on the coarse Omega, every other cell keeps its bits"""
    dt = b_f.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        t = (b_f[where_f] - q_f[where_f]).astype(dt)
        for axis in reversed(range(t.ndim)):
            t = _weigh(t, axis)
        bc, xc = b_c.copy(), x_c.copy()
        bc[where_c] = (dt(rscale) * t).astype(dt)
    xc[where_c] = dt(0)
    return bc, xc


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


def prolong_add(x_c, where_c, x_f, where_f):
    """-> a new x_f: x_f + P(x_c) on the fine Omega, every other cell keeps its bits"""
    dt = x_f.dtype.type
    e = x_c[where_c]
    for axis in reversed(range(e.ndim)):
        e = _interp(e, axis)
    out = x_f.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[where_f] = (x_f[where_f] + e).astype(dt)
    return out


# ---------------------------------------------------------------- the cycle and the solve
def sweep(L):
    L.q = L.A(L.x)
    L.x = smooth(L.q, L.b, L.minv, L.x, L.where)


def cycle(levels, l, pre, post, coarse_sweeps):
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(coarse_sweeps):
            sweep(L)
        return
    for _ in range(pre):
        sweep(L)
    L.q = L.A(L.x)
    nxt = levels[l + 1]
    nxt.b, nxt.x = restrict(L.b, L.q, L.where, L.rscale, nxt.b, nxt.x, nxt.where)
    cycle(levels, l + 1, pre, post, coarse_sweeps)
    L.x = prolong_add(nxt.x, nxt.where, L.x, L.where)
    for _ in range(post):
        sweep(L)


def residual(L):
    """-> (rr as the exact sum of the terms (b - A(x))^2 over Omega, the bound two summation orders may differ by); L.q = A(x)"""
    L.q = L.A(L.x)
    return mc.reference_sum(L.b, L.q, L.where)


def start(levels, x0, b0, work_fill=np.nan):
    """the state a solve starts from: level 0 holds the caller's x and b; the coarser x are zero-filled (whole box), the
    coarser b and every q hold `work_fill` (what the device's work fields hold before the call)"""
    for l, L in enumerate(levels):
        L.x = x0.copy() if l == 0 else np.zeros(L.shape, L.dt)
        L.b = b0.copy() if l == 0 else np.full(L.shape, work_fill, L.dt)
        L.q = np.full(L.shape, work_fill, L.dt)


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


def rr_sequence(levels, x0, b0, cycles, pre=2, post=2, coarse_sweeps=8):
    """[rr_0, rr after cycle 1, ...] as floats (the terms' exact sums)"""
    rr0, checks = run(levels, x0, b0, cycles, pre, post, coarse_sweeps, 1)
    return [rr0[0]] + [c[0] for c in checks]


def expected_stop(seq, check_every, max_cycles, tol2):
    """what the loop's definition gives on an r . r sequence: (cycles_done, checks)"""
    if seq[0] <= tol2:
        return 0, 0
    done, checks = 0, 0
    while done < max_cycles:
        done += min(check_every, max_cycles - done)
        checks += 1
        if seq[done] <= tol2:
            break
    return done, checks


def tol_between(seq, a, b):
    """a threshold at the geometric mean of seq[a] and seq[b], which must differ by at least a factor of 4: two summation
    orders move r . r by parts in 1e-13 (f64) / 1e-4 (f32), so the stop cannot hinge on rounding"""
    assert seq[b] * 4.0 <= seq[a], "precondition: consecutive check values differ by at least a factor of 4"
    return math.sqrt(seq[a] * seq[b])


# ---------------------------------------------------------------- hierarchies of the star operator
def level_shapes(omega, levels, rims=None):
    """box shapes and Omega slices of `levels` nested levels starting from interior extents `omega`; rims: per level a
    (lower, upper) pair of per-dimension rim widths (default one cell everywhere, what mg_module's bounds need)"""
    out, m = [], [int(v) for v in omega]
    for l in range(levels):
        lo, up = rims[l] if rims else ([1] * len(m), [1] * len(m))
        shape = tuple(a + n + b for a, n, b in zip(lo, m, up))
        where = tuple(slice(a, a + n) for a, n in zip(lo, m))
        out.append((shape, where))
        if l + 1 < levels:
            assert all(n % 2 == 1 and n >= 3 for n in m), m
            m = [(n - 1) // 2 for n in m]
    return out


def minv_field(shape, where, dtype, omega, outside=np.nan):
    """omega / (2 rank) on Omega (one division in the element type), `outside` elsewhere: NaN proves the rim is never used"""
    dt = np.dtype(dtype).type
    m = np.full(shape, outside, dtype)
    m[where] = dt(dt(omega) / dt(2 * len(shape)))
    return m


def star_levels(omega, n_levels, dtype, omega_damp, texts=None):
    """restatement levels of the star operator on whole-interior boxes (rim of one cell); -> (levels, module texts)"""
    shapes = level_shapes(omega, n_levels)
    texts = texts or [mg_module(shape, dtype) for shape, _ in shapes]
    levels = [Level(Operator(text), shape, where, minv_field(shape, where, dtype, omega_damp), dtype)
              for text, (shape, where) in zip(texts, shapes)]
    return levels, texts


def problem_fields(shape, where, dtype, rim=False, seed=91):
    """b (hashed) and x0: zeros, or hashed non-zero Dirichlet values on the rim with zeros inside"""
    b = helpers.hash_field(shape, dtype, seed=seed)
    x0 = np.zeros(shape, dtype)
    if rim:
        x0 = helpers.hash_field(shape, dtype, seed=seed + 1)
        x0[where] = 0
    return x0, b
