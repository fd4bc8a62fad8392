"""The NumPy restatement of semi-coarsened multigrid: mg_cases / mgcg_cases with an `axes` argument.

Between two neighbouring levels every dimension is coarsened (m_fine = 2 m_coarse + 1, today's stencils) or kept
(m_fine = m_coarse, the identity: no operation, no rounding).  restrict and prolong_add are mg_cases._weigh / _interp applied
to the listed dimensions only, in mg_cases' order (the last dimension first); with every dimension listed they are
mg_cases.restrict / prolong_add.  A level carries `axes`, the dimensions coarsened towards the next level; cycle, run and
the MGCG preconditioner / replay are those of mg_cases / mgcg_cases with the transfers above -- where mgcg_cases hard-wires
mg_cases.restrict, its few lines are restated here.

plan() restates the rule of neptune_hip.multigrid.coarsening_plan for operators -sum_d w_d u_dd on unscaled stencils with
rscale = 4; plan_levels builds the restatement's levels and module texts from it (mgcg_cases.aniso_module with the
per-level weights, damped-Jacobi weights damp / diagonal on Omega)."""
import numpy as np

import cg_cases as cc
import mg_cases as mgc
import mgcg_cases as mg

expected_stop = mgc.expected_stop
tol_between = mgc.tol_between


# ---------------------------------------------------------------- the two transfers
def restrict(b_f, q_f, where_f, rscale, b_c, x_c, where_c, axes):
    """-> new (b_c, x_c): b_c = rscale * R(b_f - q_f) and x_c = +0 on the coarse Omega, R along `axes` only; every other cell
    keeps its bits"""
    dt = b_f.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        t = (b_f[where_f] - q_f[where_f]).astype(dt)
        for axis in reversed(range(t.ndim)):
            if axis in axes:
                t = mgc._weigh(t, axis)
        bc, xc = b_c.copy(), x_c.copy()
        bc[where_c] = (dt(rscale) * t).astype(dt)
    xc[where_c] = dt(0)
    return bc, xc


def prolong_add(x_c, where_c, x_f, where_f, axes):
    """-> a new x_f: x_f + P(x_c) on the fine Omega, P along `axes` only; every other cell keeps its bits"""
    dt = x_f.dtype.type
    e = x_c[where_c]
    for axis in reversed(range(e.ndim)):
        if axis in axes:
            e = mgc._interp(e, axis)
    out = x_f.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[where_f] = (x_f[where_f] + e).astype(dt)
    return out


# ---------------------------------------------------------------- the cycle and the solve (levels carry .axes)
def cycle(levels, l, pre, post, coarse_sweeps):
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(coarse_sweeps):
            mgc.sweep(L)
        return
    for _ in range(pre):
        mgc.sweep(L)
    L.q = L.A(L.x)
    nxt = levels[l + 1]
    nxt.b, nxt.x = restrict(L.b, L.q, L.where, L.rscale, nxt.b, nxt.x, nxt.where, L.axes)
    cycle(levels, l + 1, pre, post, coarse_sweeps)
    L.x = prolong_add(nxt.x, nxt.where, L.x, L.where, L.axes)
    for _ in range(post):
        mgc.sweep(L)


def run(levels, x0, b0, cycles, pre=2, post=2, coarse_sweeps=8, check_every=1):
    """mg_cases.run on this module's cycle: -> (rr0, [rr after each block]) as (sum, bound) pairs"""
    mgc.start(levels, x0, b0)
    rr0 = mgc.residual(levels[0])
    checks, done = [], 0
    while done < cycles:
        for _ in range(min(check_every, cycles - done)):
            cycle(levels, 0, pre, post, coarse_sweeps)
            done += 1
        checks.append(mgc.residual(levels[0]))
    return rr0, checks


def rr_sequence(levels, x0, b0, cycles, pre=2, post=2, coarse_sweeps=8, stop_at=None):
    """[rr_0, rr after cycle 1, ...] as floats (the terms' exact sums); stop_at: a factor -- end early once
    rr <= stop_at * rr_0"""
    mgc.start(levels, x0, b0)
    seq = [mgc.residual(levels[0])[0]]
    for _ in range(cycles):
        if stop_at is not None and seq[-1] <= stop_at * seq[0]:
            break
        cycle(levels, 0, pre, post, coarse_sweeps)
        seq.append(mgc.residual(levels[0])[0])
    return seq


# ---------------------------------------------------------------- the MGCG preconditioner and replay
def rest_of_cycle(levels, r, z, sweeps, coarse_sweeps):
    """mgcg_cases.rest_of_cycle with the transfers above"""
    L0, L1 = levels[0], levels[1]
    L0.x, L0.b = z, r
    for _ in range(sweeps - 1):
        mgc.sweep(L0)
    L0.q = L0.A(L0.x)
    L1.b, L1.x = restrict(L0.b, L0.q, L0.where, L0.rscale, L1.b, L1.x, L1.where, L0.axes)
    cycle(levels, 1, sweeps, sweeps, coarse_sweeps)
    L0.x = prolong_add(L1.x, L1.where, L0.x, L0.where, L0.axes)
    for _ in range(sweeps):
        mgc.sweep(L0)
    return L0.x


def precondition(levels, r, sweeps=2, coarse_sweeps=8):
    """z = M(r): one V(sweeps, sweeps) cycle on A_0 z = r from z = 0 (call mgcg_cases.start(levels) once before)"""
    assert len(levels) >= 2 and sweeps >= 1
    return rest_of_cycle(levels, r, mg.first_sweep(levels, r), sweeps, coarse_sweeps)


def setup(levels, x0, b0, sweeps=2, coarse_sweeps=8):
    """mgcg_cases.setup: -> (x, r, p, z, rr0 as (terms' sum, bound), rz0 likewise)"""
    L0 = levels[0]
    mg.start(levels)
    x = x0.copy()
    q = L0.A(x)
    r = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r[L0.where] = (b0[L0.where] - q[L0.where]).astype(L0.dt)
    rr0 = cc.dot_terms(r, r, L0.where)
    z = precondition(levels, r, sweeps, coarse_sweeps)
    rz0 = cc.dot_terms(r, z, L0.where)
    return x, r, z.copy(), z, rr0, rz0


def replay(levels, x0, b0, rz0, trace, sweeps=2, coarse_sweeps=8):
    """mgcg_cases.replay: the recurrences driven by the DEVICE's scalars; -> (x, r, p, z, checks, rr0, rz0)"""
    L0 = levels[0]
    dt, where = L0.dt, L0.where
    x, r, p, z, rr0, rz0_ref = setup(levels, x0, b0, sweeps, coarse_sweeps)
    rz = dt(rz0)
    checks = []
    everywhere = tuple(slice(None) for _ in x.shape)
    for k in range(len(trace)):
        pq, rz_new = dt(trace[k][0]), dt(trace[k][1])
        q = L0.A(p)
        pq_ref = cc.dot_terms(q, p, where)
        broken = rz == 0 or pq == 0
        alpha = dt(0) if broken else dt(rz / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        rr_ref = cc.dot_terms(r, r, everywhere)
        z = precondition(levels, r, sweeps, coarse_sweeps)
        checks.append((pq_ref, cc.dot_terms(r, z, where), rr_ref))
        beta = dt(0) if broken else dt(rz_new / rz)
        p = (z + (beta * p).astype(dt)).astype(dt)
        rz = rz_new
    return x, r, p, z, checks, rr0, rz0_ref


# ---------------------------------------------------------------- hierarchies
def next_level(extents, weights, axes):
    """the plan rule's step: (m - 1) / 2 and w on a coarsened dimension, m and 4 w on a kept one"""
    assert axes and all(extents[d] % 2 == 1 and extents[d] >= 3 for d in axes), (extents, axes)
    return (tuple((m - 1) // 2 if d in axes else m for d, m in enumerate(extents)),
            tuple(w if d in axes else 4.0 * w for d, w in enumerate(weights)))


def plan(extents, weights, threshold=0.5, max_levels=16):
    """the rule of multigrid.coarsening_plan, restated: -> [(extents, weights, axes)], axes = () on the last level"""
    m, w, out = tuple(int(v) for v in extents), tuple(float(v) for v in weights), []
    while True:
        can = [d for d, v in enumerate(m) if v % 2 == 1 and v >= 3]
        if not can or len(out) + 1 >= max_levels:
            out.append((m, w, ()))
            return out
        top = max(w[d] for d in can)
        axes = tuple(d for d in can if w[d] >= threshold * top)
        out.append((m, w, axes))
        m, w = next_level(m, w, axes)


def with_axes(extents, weights, axes_per_pair):
    """[(extents, weights, axes)] for a hierarchy given by the dimensions coarsened per pair, weights by the plan rule"""
    m, w, out = tuple(int(v) for v in extents), tuple(float(v) for v in weights), []
    for axes in axes_per_pair:
        out.append((m, w, tuple(axes)))
        m, w = next_level(m, w, tuple(axes))
    out.append((m, w, ()))
    return out


def build_levels(steps, damp, dtype, outside0=0.0):
    """restatement levels (whole-interior boxes, rim of one cell) and module texts for [(extents, weights, axes)]: the
    anisotropic star with the level's weights, minv = damp / diagonal on Omega; outside Omega level 0's minv is `outside0`
    (MGCG forms minv_0 * r on the whole box), the coarser levels' NaN (never read); -> (levels, texts)"""
    dt = np.dtype(dtype).type
    levels, texts = [], []
    for l, (m, w, axes) in enumerate(steps):
        shape = tuple(n + 2 for n in m)
        where = tuple(slice(1, 1 + n) for n in m)
        text = mg.aniso_module(shape, w, dtype)
        minv = np.full(shape, outside0 if l == 0 else np.nan, dtype)
        minv[where] = dt(dt(damp) / dt(2.0 * sum(w)))
        L = mgc.Level(mgc.Operator(text), shape, where, minv, dtype)
        L.axes, L.weights = axes, w
        levels.append(L)
        texts.append(text)
    return levels, texts


def plan_levels(omega, weights, damp, dtype=np.float64, threshold=0.5, max_levels=16, outside0=0.0):
    """restatement levels and module texts from the plan rule; -> (levels, texts)"""
    return build_levels(plan(omega, weights, threshold, max_levels), damp, dtype, outside0)


def full_levels(omega, weights, damp, dtype=np.float64, outside0=0.0):
    """the fully coarsened hierarchy of the same operator (every level the same weights), down to where an extent is even
    or below 3"""
    steps, m = [], tuple(omega)
    while all(v % 2 == 1 and v >= 3 for v in m):
        steps.append(tuple(range(len(m))))
        m = tuple((v - 1) // 2 for v in m)
    return build_levels(with_axes(omega, weights, steps), damp, dtype, outside0)
