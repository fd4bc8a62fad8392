"""The NumPy restatement of the transposed linear restriction on cell-centred pairs, on mgcl_cases and its
siblings.

Along a halved dimension, a[0 .. 2 m_c) being the values after the dimensions already done, the coarse cell j takes
    s_m = 0.25 * a[2 j - 1],  p_0 = 0.75 * a[2 j],  p_1 = 0.75 * a[2 j + 1],  s_p = 0.25 * a[2 j + 2]
    u = s_m + p_0,  v = p_1 + s_p,  w = u + v,  t = 0.5 * w
in the element type with one `.astype(dt)` per operation, the last dimension first, kept dimensions skipped; a[-1] and
a[2 m_c] are the ghosts +a[edge] (EVEN) / -a[edge] (ODD): the FINE intermediate array padded with +- its own edge, which is
what include/neptune_hip.h defines and exactly the transpose of padding the coarse array in mgcl_cases._linear.

A pair carries a Transfers(axes, rim, prolong, restrict) -- an mgcc_cases.Halved with the one rule array .rim[d] = (low rule,
high rule) that serves BOTH transfers, .prolong = "constant" | "linear" and .restrict = "average" | "linear".  restrict and
prolong_add dispatch on that marker and hand every other pair to mgcl_cases.  The cycle, the run, the MGCG preconditioner, the
set-up and the replay from traced scalars are mgsemi_cases' own functions (numpy_mgcg is mgcg_cases') re-bound to this
module's namespace, as mgcc_cases and mgcl_cases re-bind them; `composed` holds mgfuzz_cases' composed restatement (line
stages per level, one-type or mixed precision) re-bound the same way.  Nothing of them is written twice."""
import types

import numpy as np

import cg_cases as cc          # the name mgsemi_cases' functions look up for dot_terms
import mg_cases as mgc
import mgcc_cases as mcc
import mgcg_cases as mg
import mgcl_cases as cl
import mgfuzz_cases as fz
import mgsemi_cases as sc
from mgcc_cases import Halved
from mgcl_cases import EVEN, ODD, complement, rim_of

expected_stop = mgc.expected_stop
tol_between = mgc.tol_between
flux_levels = cl.flux_levels
star_levels = cl.star_levels
problem = cl.problem


class Transfers(Halved):
    """the dimensions halved between a level and the next one, both transfers chosen: .prolong, .restrict and the one rule
    array .rim[d] = (low, high) rule of dimension d that serves both"""

    def __new__(cls, axes, rim, prolong="linear", restrict="linear"):
        self = super().__new__(cls, axes)
        self.rim = tuple((int(lo), int(hi)) for lo, hi in rim)
        assert all(v in (EVEN, ODD) for pair in self.rim for v in pair)
        assert prolong in ("constant", "linear") and restrict in ("average", "linear")
        self.prolong, self.restrict = prolong, restrict
        return self

    @property
    def symmetric(self):
        return (self.prolong == "linear") == (self.restrict == "linear")


# ---------------------------------------------------------------- the restriction
def _gather(a, axis, rule_lo, rule_hi):
    """2 m -> m cells along `axis`: the four operands a[2 j - 1 .. 2 j + 2] with the weights 1/4, 3/4, 3/4, 1/4, a padded with
    + (EVEN) or - (ODD) its own edge"""
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


def restrict_linear(b_f, q_f, where_f, rscale, b_c, x_c, where_c, axes, rim):
    """-> new (b_c, x_c): b_c = rscale * R(b_f - q_f) and x_c = +0 on the coarse Omega, R = P^T / 2 along each of `axes` by the
    rules rim[d] = (low, high); every other cell keeps its bits; nothing outside where_f is read"""
    dt = b_f.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        t = (b_f[where_f] - q_f[where_f]).astype(dt)
        for axis in reversed(range(t.ndim)):
            if axis in axes:
                t = _gather(t, axis, *rim[axis])
        bc, xc = b_c.copy(), x_c.copy()
        bc[where_c] = (dt(rscale) * t).astype(dt)
    xc[where_c] = dt(0)
    return bc, xc


def restrict(b_f, q_f, where_f, rscale, b_c, x_c, where_c, axes):
    if isinstance(axes, Transfers) and axes.restrict == "linear":
        return restrict_linear(b_f, q_f, where_f, rscale, b_c, x_c, where_c, axes, axes.rim)
    return cl.restrict(b_f, q_f, where_f, rscale, b_c, x_c, where_c, axes)


def prolong_add(x_c, where_c, x_f, where_f, axes):
    if isinstance(axes, Transfers):
        if axes.prolong == "linear":
            return cl.prolong_add_linear(x_c, where_c, x_f, where_f, axes, axes.rim)
        return mcc.prolong_add_cell(x_c, where_c, x_f, where_f, axes)
    return cl.prolong_add(x_c, where_c, x_f, where_f, axes)


# ---------------------------------------------------------------- the cycle, the solve, the MGCG preconditioner and replay
def _rebound(fn, namespace=None):
    out = types.FunctionType(fn.__code__, globals() if namespace is None else namespace, fn.__name__, fn.__defaults__)
    out.__doc__ = fn.__doc__
    return out


cycle = _rebound(sc.cycle)
run = _rebound(sc.run)
rr_sequence = _rebound(sc.rr_sequence)
rest_of_cycle = _rebound(sc.rest_of_cycle)
precondition = _rebound(sc.precondition)
setup = _rebound(sc.setup)
replay = _rebound(sc.replay)
_sum = mg._sum
numpy_mgcg = _rebound(mg.numpy_mgcg)

# mgfuzz_cases' composed restatement (a level may carry .stages; a problem may be an mgcgmixed_cases.Problem) calls
# cc.restrict / cc.prolong_add: its globals with `cc` = this module's two transfers
_composed = dict(vars(fz))
_composed["cc"] = types.SimpleNamespace(restrict=restrict, prolong_add=prolong_add)
for _name in ("descend", "cycle", "run", "rest_of_cycle", "precondition", "setup", "replay"):
    _composed[_name] = _rebound(getattr(fz, _name), _composed)
composed = types.SimpleNamespace(**{_name: _composed[_name] for _name in ("cycle", "run", "precondition", "setup", "replay")})
lines_run = composed.run


# ---------------------------------------------------------------- hierarchies
def transfer_steps(steps, rim, prolong="linear", restrict="linear", only=None):
    """mgcc_cases' steps [(extents, weights, axes)] with every Halved pair (or the pairs listed in `only`) made a
    Transfers(axes, rim, prolong, restrict)"""
    out = []
    for l, (m, w, axes) in enumerate(steps):
        if isinstance(axes, Halved) and len(axes) and (only is None or l in only):
            axes = Transfers(axes, rim, prolong, restrict)
        out.append((m, w, axes))
    return out


def transfer_of(axes, rank):
    """(prolong kind, restrict kind, low rules, high rules) of a level's .axes as neptune_hip_mg_transfer_t holds them"""
    if isinstance(axes, Transfers):
        kinds = (int(axes.prolong == "linear"), int(axes.restrict == "linear"))
        rim = axes.rim
    elif isinstance(axes, cl.Linear):
        kinds, rim = (1, 0), axes.rim
    else:
        kinds, rim = (0, 0), ((EVEN, EVEN),) * rank
    return kinds + ([lo for lo, _ in rim], [hi for _, hi in rim])


FACE = {EVEN: "neumann", ODD: "dirichlet"}


def faces_of(rim):
    """the Python layer's faces= for a rule array"""
    return [(FACE[lo], FACE[hi]) for lo, hi in rim]


def mgcg_iterations(steps, faces, damp, sweeps, factor=1e-16, coarse_sweeps=8, dtype=np.float64, max_iters=60):
    """the iteration at which numpy_mgcg on flux_levels(steps, faces) first has r . r <= factor * rr_0, from x = 0 and
    mgcl_cases.problem's b"""
    levels, _, _ = flux_levels(steps, damp, dtype, faces)
    x0, b = problem(levels, faces, dtype)
    L0 = levels[0]
    r0 = b.copy()
    rr0 = float(_sum((r0[L0.where] * r0[L0.where]).astype(L0.dt)))
    seq = numpy_mgcg(levels, x0, b, max_iters, sweeps, coarse_sweeps, stop_at=factor * rr0)
    assert seq[-1] <= factor * seq[0], "not converged"
    return len(seq) - 1
