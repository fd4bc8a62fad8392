"""Composed multigrid hierarchies, fuzzed: ONE NumPy restatement of the cycle, the solve, the MGCG
preconditioner and the replay, composed of the pieces the features' own case modules define, and a seeded generator of
hierarchies that mix what those modules test one at a time.

First half -- the restatement.  Nothing of the arithmetic is written again: the transfers are mgcc_cases.restrict /
prolong_add (they dispatch per pair on Level.axes: an mgcc_cases.Halved goes to the cell-centred pair, a plain tuple to
mgsemi_cases' vertex-centred one, mg_cases._weigh / _interp underneath), the sweep is mglines_cases.sweep (line_stage on a
level with stages, mg_cases.smooth on one without, the stages reversed for a post-sweep), the first pre-sweep of the
preconditioner is mgcglines_cases.first_stage or mgcg_cases.first_sweep, the recurrences are those of mgcg_cases.replay,
and the mixed form narrows, widens and updates with mgcgmixed_cases.  Only the control flow of include/neptune_hip.h --
Cycle(l), "the rest of M", the set-up, the iteration -- stands here, once.

A level's operator is OmegaOperator: the oracle's A on Omega and +0 on every other cell.  That is what q holds where the
solvers read it outside Omega: the MGCG drivers stream q over the whole box, a launch writes Omega (and copies p = +0
through between the launch region and the module's bounds), and where the region is not the whole box the drivers zero-fill
q once.  Sweeps, stages and transfers read q on Omega only.

Second half -- the generator.  decode(seed) draws a case from a fixed pool of module templates (TEMPLATES): a template fixes
rank, element type, the boxes (unequal rims of 1..3 cells), the modules' bounds and, per pair, the dimensions transferred --
so also the weights per level, by the plan rule (w on a transferred dimension, 4 w on a kept one).  Everything else is drawn
and costs no compile: how many of the template's levels are used, Omega inside the bounds (a launch region), and with it the
GRID KIND of every pair -- bounds of 264 -> 132 -> 66 -> 33 hold 264 -> 132 -> 66 -> 33 (halved), 263 -> 131 -> 65 -> 32
(coarsened), 262 -> 131 -> 65 and 261 -> 130 -> 65 (the kind switches) --, the line stages per level, the schedule, the launch
path and the allocation offset.  build(case) makes the restatement's levels and the problem's fields."""
import sys

import numpy as np

import cg_cases as cgc
import helpers
import mg_cases as mgc
import mgcc_cases as cc
import mgcg_cases as mg
import mgcglines_cases as mlc
import mgcgmixed_cases as mx
import mglines_cases as lc
import monitor_cases as mc
from mgcc_cases import Halved

D, S = np.float64, np.float32
DAMP = 0.8


# ================================================================ first half: the composed restatement
class OmegaOperator:
    """the oracle's A for one module text, on Omega: q = A(u) on `where`, +0 on every other cell (module docstring)"""
    _parsed = {}

    def __init__(self, text, where):
        if text not in self._parsed:
            self._parsed[text] = mgc.Operator(text)
        self.A, self.where, self.rest = self._parsed[text], tuple(where), ()

    def __call__(self, u):
        out = np.zeros_like(u)
        out[self.where] = self.A(u)[self.where]
        return out


def axes_of(L):
    """the dimensions transferred between L and the next level: L.axes (a Halved for a cell-centred pair), default all"""
    return getattr(L, "axes", tuple(range(len(L.shape))))


sweep = lc.sweep        # stages 0 .. k-1 (reverse: k-1 .. 0), each after its own apply; without stages mg_cases.sweep


def descend(levels, l, pre, post, coarse_sweeps):
    """q = A(x) and the restriction; Cycle(l + 1); prolongation and correction"""
    L, nxt = levels[l], levels[l + 1]
    L.q = L.A(L.x)
    nxt.b, nxt.x = cc.restrict(L.b, L.q, L.where, L.rscale, nxt.b, nxt.x, nxt.where, axes_of(L))
    cycle(levels, l + 1, pre, post, coarse_sweeps)
    L.x = cc.prolong_add(nxt.x, nxt.where, L.x, L.where, axes_of(L))


def cycle(levels, l, pre, post, coarse_sweeps):
    """Cycle(l) of include/neptune_hip.h"""
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


def run(levels, x0, b0, cycles, pre=2, post=2, coarse_sweeps=8, check_every=1):
    """the solve with no tolerance: -> (rr0, [rr after each block]) as (sum, bound) pairs; the fields are left in `levels`"""
    mgc.start(levels, x0, b0)
    rr0 = mgc.residual(levels[0])
    checks, done = [], 0
    while done < cycles:
        for _ in range(min(check_every, cycles - done)):
            cycle(levels, 0, pre, post, coarse_sweeps)
            done += 1
        checks.append(mgc.residual(levels[0]))
    return rr0, checks


def first_pre_sweep(levels, r):
    """level 0's first pre-sweep on (x, b) = (z, r) from z = 0: with stages, stage 0 apply-free and the others plain; without,
    z = minv_0 * r on every cell"""
    L0 = levels[0]
    stages = getattr(L0, "stages", [])
    L0.b = r
    if not stages:
        L0.x = mg.first_sweep(levels, r)
        return
    axis, lo, inv, up = stages[0]
    L0.x = mlc.first_stage(r, lo, inv, up, np.zeros(L0.shape, L0.dt), L0.where, axis)
    for axis, lo, inv, up in stages[1:]:
        L0.q = L0.A(L0.x)
        L0.x = lc.line_stage(L0.q, L0.b, lo, inv, up, L0.x, L0.where, axis)


def rest_of_cycle(levels, sweeps, coarse_sweeps):
    """"the rest of M": everything of the cycle on level 0's (x, b) = (z, r) after its first pre-sweep; -> z"""
    L0 = levels[0]
    for _ in range(sweeps - 1):
        sweep(L0)
    descend(levels, 0, sweeps, sweeps, coarse_sweeps)
    for _ in range(sweeps):
        sweep(L0, reverse=True)
    return L0.x


def precondition(levels, r, sweeps=2, coarse_sweeps=8):
    """z = M(r): one V(sweeps, sweeps) cycle on A_0 z = r from z = 0 (call mgcg_cases.start(levels) once before)"""
    assert len(levels) >= 2 and sweeps >= 1
    first_pre_sweep(levels, r)
    return rest_of_cycle(levels, sweeps, coarse_sweeps)


class State:
    """the fields of an MGCG run: x, r, p, z (mixed: x, r, p in f64 and r32, z32)"""


def setup(problem, x0, b0, sweeps=2, coarse_sweeps=8):
    """the definition's set-up for a list of levels or an mgcgmixed_cases.Problem: -> (State, rr0, rz0), the two sums as
    (terms' sum, bound)"""
    st = State()
    if isinstance(problem, mx.Problem):
        st.x, st.r, st.r32, z32, rr0 = mx.store_residual(problem, x0, b0)
        L0 = problem.levels[0]
        L0.x, L0.b = z32, st.r32
        st.z32 = rest_of_cycle(problem.levels, sweeps, coarse_sweeps)
        st.p = mx.widen(st.z32)
        return st, rr0, mx.wide_dot_terms(st.r32, st.z32, problem.where)
    L0 = problem[0]
    mg.start(problem)
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
    """numpy's own sum of the terms in their element type, as mgcg_cases.numpy_mgcg forms its scalars"""
    return terms.dtype.type(np.sum(terms, dtype=terms.dtype))


def replay(problem, x0, b0, rz0=None, trace=None, sweeps=2, coarse_sweeps=8, iters=None):
    """The recurrences of mgcg_cases.replay / mgcgmixed_cases.replay on the composed preconditioner, driven by the DEVICE's
    scalars rz0 and trace rows (pq_k, rz_(k+1), rr_(k+1)) -- or, with trace = None, by numpy's own sums for `iters`
    iterations, as numpy_mgcg.  -> (State, checks, rr0, rz0_ref, scalars): checks[k] = the (terms' sum, bound) pairs of pq,
    rz' and rr' of the replay's own fields; scalars[k] = (pq, rz', rr', broken) as used; the levels' x_l, b_l are left in the
    levels."""
    mixed = isinstance(problem, mx.Problem)
    A = problem.A if mixed else problem[0].A
    where = problem.where if mixed else problem[0].where
    dt = D if mixed else problem[0].dt
    st, rr0, rz0_ref = setup(problem, x0, b0, sweeps, coarse_sweeps)
    zr = (lambda: (mx.widen(st.r32[where]) * mx.widen(st.z32[where]))) if mixed else (lambda: (st.r[where] * st.z[where]).astype(dt))
    rz = dt(rz0) if trace is not None else _own(zr())
    st.rz0_used = rz
    checks, scalars = [], []
    everywhere = tuple(slice(None) for _ in st.x.shape)
    for k in range(len(trace) if trace is not None else iters):
        q = A(st.p)
        pq_ref = cgc.dot_terms(q, st.p, where)
        pq = dt(trace[k][0]) if trace is not None else _own((q[where] * st.p[where]).astype(dt))
        broken = rz == 0 or pq == 0
        alpha = dt(0) if broken else dt(rz / pq)
        if mixed:
            st.x, st.r, st.r32, z32 = mx.update(problem, alpha, st.x, st.r, st.p, q)
            L0 = problem.levels[0]
            L0.x, L0.b = z32, st.r32
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                st.x = (st.x + (alpha * st.p).astype(dt)).astype(dt)
                st.r = (st.r - (alpha * q).astype(dt)).astype(dt)
        rr_ref = cgc.dot_terms(st.r, st.r, everywhere)
        if mixed:
            st.z32 = rest_of_cycle(problem.levels, sweeps, coarse_sweeps)
            rz_ref = mx.wide_dot_terms(st.r32, st.z32, where)
        else:
            st.z = precondition(problem, st.r, sweeps, coarse_sweeps)
            rz_ref = cgc.dot_terms(st.r, st.z, where)
        checks.append((pq_ref, rz_ref, rr_ref))
        rz_new = dt(trace[k][1]) if trace is not None else _own(zr())
        beta = dt(0) if broken else dt(rz_new / rz)
        with np.errstate(invalid="ignore", over="ignore"):
            st.p = ((mx.widen(st.z32) if mixed else st.z) + (beta * st.p).astype(dt)).astype(dt)
        scalars.append((pq, rz_new, _own((st.r * st.r).astype(dt)), bool(broken)))
        rz = rz_new
    return st, checks, rr0, rz0_ref, scalars


# ================================================================ second half: the seeded generator
# name: (element type of the hierarchy, [the module's bounds extents per level], [the dimensions transferred per pair],
#        whether an f64 outer operator of level 0 exists (mixed precision))
# Transferred extents double from level to level (or double plus one), kept ones stay: Omega, drawn inside the bounds,
# decides the grid kind of a pair.  The contiguous chains are the ones that cross the 256-cell chunk with a short tail
# (264 / 263 / 262 / 261), the short ones give rows below a wave and levels of one or two cells.
TEMPLATES = {
    "r1_long":   (D, [(264,), (132,), (66,), (33,)], [(0,)] * 3, False),
    "r1_short":  (S, [(16,), (8,), (4,), (2,)], [(0,)] * 3, False),
    "r2_odd":    (D, [(15, 263), (7, 131), (3, 65), (1, 32)], [(0, 1)] * 3, False),
    "r2_semi":   (S, [(14, 264), (14, 132), (7, 66), (7, 33)], [(1,), (0, 1), (1,)], True),
    "r2_lines":  (D, [(70, 16), (70, 8), (70, 4)], [(1,), (1,)], False),
    "r2_even":   (S, [(16, 264), (8, 132), (4, 66)], [(0, 1)] * 2, True),
    "r3_even":   (D, [(8, 16, 264), (4, 8, 132), (2, 4, 66)], [(0, 1, 2)] * 2, False),
    "r3_odd":    (S, [(7, 15, 263), (3, 7, 131), (1, 3, 65)], [(0, 1, 2)] * 2, True),
    "r3_2":      (D, [(3, 7, 264), (3, 7, 132)], [(2,)], False),
    "r3_1":      (S, [(2, 14, 70), (2, 7, 70)], [(1,)], False),
    "r3_0":      (D, [(14, 3, 33), (7, 3, 33)], [(0,)], False),
    "r3_01":     (S, [(6, 14, 15), (3, 7, 15)], [(0, 1)], False),
    "r3_02":     (D, [(6, 1, 264), (3, 1, 132)], [(0, 2)], False),
    "r3_12":     (S, [(1, 16, 32), (1, 8, 16)], [(1, 2)], False),
}
FORMS = {0: "solve", 1: "cg", 2: "cg-lines", 3: "mixed", 9: "refused"}
REFUSALS = ("mixed_kinds", "mixed_stage0", "stage_axis")


def seed_class(seed):
    """the form a seed draws: the thousands say it"""
    return FORMS[seed // 1000]


def template_levels(name):
    """-> per level (box shape, bounds (lb, ub), weights): rims of 1..3 cells, unequal, fixed per level and dimension"""
    _, extents, transferred, _ = TEMPLATES[name]
    rank = len(extents[0])
    w, out = tuple(1.0 for _ in range(rank)), []
    for l, B in enumerate(extents):
        lo = [1 + (l + d) % 3 for d in range(rank)]
        hi = [1 + (l + 2 * d + 1) % 3 for d in range(rank)]
        shape = tuple(a + n + b for a, n, b in zip(lo, B, hi))
        out.append((shape, (lo, [a + n for a, n in zip(lo, B)]), w))
        if l + 1 < len(extents):
            w = tuple(v if d in transferred[l] else 4.0 * v for d, v in enumerate(w))
    return out


def module_text(name, level, dtype):
    """the operator -sum_d w_d u_dd of a template's level, unscaled: monitor_cases.star_module where all weights are equal,
    mgcg_cases.aniso_module otherwise"""
    shape, bounds, w = template_levels(name)[level]
    if len(set(w)) == 1:
        return mc.star_module(shape, dtype, bounds=bounds, centre=2.0 * len(shape) * w[0], side=-w[0])
    return mg.aniso_module(shape, w, dtype, bounds=bounds)


def case_modules(case):
    """[(module text, compiled with its dot entry)] of a case: the outer operator of a mixed case first, then the levels;
    level 0 of every template is compiled with its dot entry (the CG forms need it, solve() launches the plain entry of the
    same object)"""
    name = case["template"]
    out = [(module_text(name, 0, D), True)] if case["form"] == "mixed" or case.get("why") == "mixed_stage0" else []
    return out + [(module_text(name, l, case["dtype"]), l == 0) for l in range(case["n_levels"])]


def _native_kinds(extents, transferred):
    """the grid kind of each pair when Omega is the bounds themselves; None when the bounds do not nest"""
    kinds = []
    for l, axes in enumerate(transferred):
        ks = {"H" if extents[l][d] == 2 * extents[l + 1][d] else "C" if extents[l][d] == 2 * extents[l + 1][d] + 1 else "?" for d in axes}
        if len(ks) != 1 or "?" in ks or any(extents[l][d] != extents[l + 1][d] for d in range(len(extents[0])) if d not in axes):
            return None
        kinds.append(ks.pop())
    return kinds


def _chain(m_last, transferred, kinds):
    """Omega's extents per level from the coarsest upward: 2 m + 1 (coarsened), 2 m (halved) or m (kept)"""
    out = [tuple(m_last)]
    for axes, kind in zip(reversed(transferred), reversed(kinds)):
        out.append(tuple((2 * m + (kind == "C") if d in axes else m) for d, m in enumerate(out[-1])))
    return out[::-1]


def decode(seed):
    """the full description of a case, a dict of plain values; deterministic"""
    rng = np.random.default_rng(seed)
    form = seed_class(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    case = {"seed": seed, "form": form}
    if form == "refused":
        why = REFUSALS[seed % len(REFUSALS)]
        name = {"mixed_kinds": "r3_01", "mixed_stage0": "r2_even", "stage_axis": "r2_odd"}[why]
        dtype, extents, transferred, _ = TEMPLATES[name]
        n_levels = 2
        m = [extents[0], extents[1]]
        stages = [[], []]
        if why == "mixed_kinds":        # dimension 0 halved, 6 -> 3, and dimension 1 coarsened, 13 -> 6, in one pair
            m = [(6, 13, 15), (3, 6, 15)]
        elif why == "mixed_stage0":
            stages = [[1], [0]]
        else:
            stages = [[], [len(extents[0])]]
        kinds = ["H" if why != "stage_axis" else "C"]
        case.update(why=why)
    else:
        names = sorted(TEMPLATES)
        if form == "mixed":
            names = [n for n in names if TEMPLATES[n][3]]
        name = pick(names)
        dtype, extents, transferred, _ = TEMPLATES[name]
        n_levels = int(rng.integers(2, len(extents) + 1))
        extents, transferred = extents[:n_levels], transferred[:n_levels - 1]
        rank = len(extents[0])
        native = _native_kinds(extents, transferred)
        assert native is not None, name
        narrowed = bool(rng.integers(2))
        m, kinds = list(extents), native
        for _ in range(64 if narrowed else 0):
            ks = [pick("CH") for _ in transferred]
            last = [int(rng.integers(1, B + 1)) if B <= 4 else int(B - rng.integers(0, 3)) for B in extents[-1]]
            cand = _chain(last, transferred, ks)
            if min(last) >= 1 and all(v <= B for mm, BB in zip(cand, extents) for v, B in zip(mm, BB)) and cand != list(extents):
                m, kinds = cand, ks
                break
        k0 = {"cg": (0, 0), "mixed": (0, 0), "cg-lines": (1, 3)}.get(form)
        stages = []
        for l in range(n_levels):
            k = int(rng.integers(k0[0], k0[1] + 1)) if (k0 and l == 0) else int(pick((0, 0, 0, 1, 1, 2, 3)))
            stages.append([int(rng.integers(rank)) for _ in range(k)])
    levels = template_levels(name)
    lo = []
    for l in range(n_levels):
        lb = levels[l][1][0]
        lo.append(tuple(int(a + rng.integers(0, B - v + 1)) for a, B, v in zip(lb, TEMPLATES[name][1][l], m[l])))
    case.update(template=name, rank=len(m[0]), dtype=dtype, n_levels=n_levels, kinds=list(kinds),
                transferred=[tuple(a) for a in TEMPLATES[name][2][:n_levels - 1]], m=[tuple(v) for v in m], lo=lo,
                shapes=[levels[l][0] for l in range(n_levels)], bounds=[levels[l][1] for l in range(n_levels)],
                weights=[levels[l][2] for l in range(n_levels)], stages=stages,
                narrowed=[tuple(m[l]) != tuple(TEMPLATES[name][1][l]) for l in range(n_levels)])
    pre, post = pick(((0, 1), (0, 2), (1, 0), (2, 0), (1, 1), (1, 2), (2, 1), (2, 2)))
    case.update(pre=int(pre), post=int(post), sweeps=int(rng.integers(1, 3)), coarse_sweeps=int(rng.integers(1, 9)),
                n=int(rng.integers(1, 4)), check_every=int(rng.integers(1, 4)), graph=bool(rng.integers(2)),
                offset=int(8 * rng.integers(2)), both_paths=seed % 4 == 0)
    # one solve() case in eight works on subnormal numbers (x0 and b scaled by a power of two): a transfer that scales before
    # it adds, or a kernel that flushes, shows there and only there.  (The CG forms divide by sums of squares: not for them.)
    case["tiny"] = bool(form == "solve" and rng.integers(8) == 0)
    return case


def where_of(case, l):
    return tuple(slice(a, a + v) for a, v in zip(case["lo"][l], case["m"][l]))


def region_of(case, l):
    """the launch region that narrows the module's bounds to Omega (result-physical), None where Omega is the bounds: along a
    narrowed dimension Omega's own range, along the others the whole box"""
    if not case["narrowed"][l]:
        return None
    lb, ub = case["bounds"][l]
    cut = [v != b - a for v, a, b in zip(case["m"][l], lb, ub)]
    return ([a if c else 0 for a, c in zip(case["lo"][l], cut)],
            [a + v if c else n for a, v, c, n in zip(case["lo"][l], case["m"][l], cut, case["shapes"][l])])


def stage_factors(shape, where, weights, axis, dtype, outside=np.nan):
    """(axis, lo, inv, up): mglines_cases.factors on the tridiagonal part (-w_a, 2 sum w, -w_a) of the operator along `axis`
    over Omega, the couplings to cells outside Omega dropped; `outside` on every cell outside Omega"""
    lower, diag, upper = (np.zeros(shape, dtype) for _ in range(3))
    lower[where], diag[where], upper[where] = -weights[axis], 2.0 * sum(weights), -weights[axis]
    first, last = list(where), list(where)
    first[axis], last[axis] = where[axis].start, where[axis].stop - 1
    lower[tuple(first)] = 0.0
    upper[tuple(last)] = 0.0
    return (axis,) + lc.factors(lower, diag, upper, where, axis, DAMP, outside)


def restatement_levels(case, dtype=None):
    """the restatement's levels of a case (mg_cases.Level with .axes, .stages, .weights): minv = DAMP / diagonal on Omega; outside
    Omega level 0's is +0 for the CG forms (they form minv_0 * r on the whole box) and NaN everywhere else, as the factor fields"""
    dtype = dtype or case["dtype"]
    dt = np.dtype(dtype).type
    name, levels = case["template"], []
    for l in range(case["n_levels"]):
        shape, where, w = case["shapes"][l], where_of(case, l), case["weights"][l]
        zero_outside = l == 0 and case["form"] in ("cg", "cg-lines", "mixed")
        minv = np.full(shape, 0.0 if zero_outside else np.nan, dtype)
        minv[where] = dt(dt(DAMP) / dt(2.0 * sum(w)))
        L = mgc.Level(OmegaOperator(module_text(name, l, dtype), where), shape, where, minv, dtype)
        L.weights = w
        if l + 1 < case["n_levels"]:
            L.axes = Halved(case["transferred"][l]) if case["kinds"][l] == "H" else tuple(case["transferred"][l])
        else:
            L.axes = ()
        L.stages = [stage_factors(shape, where, w, a, dtype) for a in case["stages"][l] if a < len(shape)]   # (a refused case's axis)
        levels.append(L)
    return levels


def problem_fields(case):
    """x0: hashed non-zero values outside Omega_0 and +0 inside; b: hashed, every 7th cell a -0; both read-only"""
    dtype = D if case["form"] == "mixed" or case.get("why") == "mixed_stage0" else case["dtype"]
    shape, where = case["shapes"][0], where_of(case, 0)
    x0 = helpers.hash_field(shape, dtype, seed=case["seed"] + 1)
    assert (x0 != 0).all()
    x0[where] = 0.0
    b = helpers.hash_field(shape, dtype, seed=case["seed"] + 2)
    b.reshape(-1)[case["seed"] % 7::7] = -0.0
    if case["tiny"]:            # |values| < 2^-140 (f32) or 2^-1065 (f64): all subnormal, nine or so bits each
        scale = np.dtype(dtype).type(2.0) ** (-140 if np.dtype(dtype) == S else -1065)
        x0, b = x0 * scale, b * scale
    for a in (x0, b):
        a.setflags(write=False)
    return x0, b


class Built:
    """a case ready to run: .case, .levels (the restatement's; f32 for a mixed case), .problem (what setup / replay take: the
    levels, or an mgcgmixed_cases.Problem around them), .x0, .b"""


def build(case):
    B = Built()
    B.case = case
    B.levels = restatement_levels(case)
    B.problem = B.levels
    if case["form"] == "mixed":
        B.problem = mx.Problem(OmegaOperator(module_text(case["template"], 0, D), B.levels[0].where), B.levels)
    B.x0, B.b = problem_fields(case)
    return B


def reference(B):
    """the restatement's solve() run of a built case: -> (rr0, checks); the fields are left in B.levels"""
    c = B.case
    return run(B.levels, B.x0, B.b, c["n"], c["pre"], c["post"], c["coarse_sweeps"], c["check_every"])


def expected_counts(case):
    """(plain, graph, checks) of solve() / (plain, graph, checks) of cg_solve for `n` cycles or iterations with no tolerance:
    the first runs as plain launches, and when at least two more may follow one is captured and every later one replays it"""
    n = case["n"]
    plain = n if (not case["graph"] or n < 3) else 1
    return plain, n - plain, -(-n // case["check_every"])


# the seed list: chosen so that tests/test_mgfuzz_host.py's coverage items all hold (a seed taken out fails there)
SEEDS = [0, 5, 38, 41, 49, 67, 71, 82, 95, 102, 122, 123, 166, 191, 222, 266, 276, 291, 293, 299, 308, 352,      # solve
         1006, 1010, 1026, 1057, 1068, 1070, 1092, 1175, 1201, 1350,                                              # cg
         2021, 2023, 2030, 2046, 2056, 2264, 2274, 2296,                                                          # cg-lines
         3006, 3007, 3024, 3047, 3090, 3196, 3225, 3352,                                                          # mixed
         9000, 9001, 9002]                                                                                        # refused


def describe(seed):
    case = decode(seed)
    lines = [f"seed {seed}: {case['form']}" + (f" ({case['why']})" if "why" in case else "") +
             f", template {case['template']}, rank {case['rank']}, {np.dtype(case['dtype']).name}, {case['n_levels']} levels"]
    for l in range(case["n_levels"]):
        pair = f"  -> {case['kinds'][l]} along {case['transferred'][l]}" if l + 1 < case["n_levels"] else ""
        lines.append(f"  level {l}: box {case['shapes'][l]}, bounds {case['bounds'][l]}, Omega {case['m'][l]} at {case['lo'][l]}, "
                     f"region {region_of(case, l)}, weights {case['weights'][l]}, stages {case['stages'][l]}{pair}")
    lines.append("  " + ", ".join(f"{k} = {case[k]}" for k in ("pre", "post", "sweeps", "coarse_sweeps", "n", "check_every", "graph",
                                                               "offset", "both_paths", "tiny")))
    return "\n".join(lines)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--describe":
        print(describe(int(sys.argv[2])))
    else:
        print("usage: python tests/mgfuzz_cases.py --describe SEED")
