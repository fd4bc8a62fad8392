"""The NumPy restatement of multigrid-preconditioned conjugate gradients with line stages (neptune_hip_mgcg_solve_lines,
DESIGN 3.18), composed of mglines_cases (the line stage, the sweep order, the cycle) and mgcg_cases (the CG recurrences and
the trace-replay pattern).

Everything follows the normative definition in include/neptune_hip.h: arithmetic in the element type with one `.astype(dt)`
per operation, the operator itself from the oracle.  A level is an mg_cases.Level with `.stages` (mglines_cases).  When
level 0 has stages the preconditioner z = M(r) is one V(sweeps, sweeps) cycle of mglines_cases on A z = r from z = 0 whose very
first stage runs no apply (first_stage) and whose very last stage also yields r . z; without stages on level 0 it is
mgcg_cases' preconditioner (z = minv_0 * r first) over mglines_cases' cycle on the coarser levels.  The sums are compared as
exact sums of the restatement's own terms (cg_cases.dot_terms); the fields, driven by the device's traced scalars, bit for
bit."""
import numpy as np

import cg_cases as cc
import mgcg_cases as mg
import mglines_cases as lc
import mgsemi_cases as sc

expected_stop = mg.expected_stop
tol_between = mg.tol_between
start = mg.start


# ---------------------------------------------------------------- the apply-free stage
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


# ---------------------------------------------------------------- the preconditioner
def rest_of_cycle(levels, sweeps, coarse_sweeps):
    """everything of the cycle on level 0's (x, b) = (z, r) after its first pre-sweep: the other pre-sweeps (stages 0 .. k-1),
    the coarser levels, the post-sweeps (stages k-1 .. 0); -> z"""
    L0, L1 = levels[0], levels[1]
    for _ in range(sweeps - 1):
        lc.sweep(L0)
    L0.q = L0.A(L0.x)
    axes = getattr(L0, "axes", tuple(range(len(L0.shape))))
    L1.b, L1.x = sc.restrict(L0.b, L0.q, L0.where, L0.rscale, L1.b, L1.x, L1.where, axes)
    lc.cycle(levels, 1, sweeps, sweeps, coarse_sweeps)
    L0.x = sc.prolong_add(L1.x, L1.where, L0.x, L0.where, axes)
    for _ in range(sweeps):
        lc.sweep(L0, reverse=True)
    return L0.x


def precondition(levels, r, sweeps=2, coarse_sweeps=8):
    """z = M(r) (call start(levels) once before).  Level 0 with stages: from z = +0 on the whole box, stage 0 apply-free,
    stages 1 .. k-1 of the first pre-sweep plain; without: z = minv_0 * r on every cell."""
    assert len(levels) >= 2 and sweeps >= 1
    L0 = levels[0]
    stages = getattr(L0, "stages", [])
    L0.b = r
    if stages:
        axis, lo, inv, up = stages[0]
        L0.x = first_stage(r, lo, inv, up, np.zeros(L0.shape, L0.dt), L0.where, axis)
        for axis, lo, inv, up in stages[1:]:
            L0.q = L0.A(L0.x)
            L0.x = lc.line_stage(L0.q, L0.b, lo, inv, up, L0.x, L0.where, axis)
    else:
        L0.x = mg.first_sweep(levels, r)
    return rest_of_cycle(levels, sweeps, coarse_sweeps)


# ---------------------------------------------------------------- the solve
def setup(levels, x0, b0, sweeps=2, coarse_sweeps=8):
    """the definition's set-up: -> (x, r, p, z, rr0 as (terms' sum, bound), rz0 likewise)"""
    L0 = levels[0]
    start(levels)
    x = x0.copy()
    q = L0.A(x)
    r = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r[L0.where] = (b0[L0.where] - q[L0.where]).astype(L0.dt)
    rr0 = cc.dot_terms(r, r, L0.where)
    z = precondition(levels, r, sweeps, coarse_sweeps)
    rz0 = cc.dot_terms(r, z, L0.where)
    return x, r, z.copy(), z, rr0, rz0


def numpy_mgcg(levels, x0, b0, iters, sweeps=2, coarse_sweeps=8, stop_at=None):
    """mgcg_cases.numpy_mgcg on this module's preconditioner: -> the r . r sequence [rr_0, rr_1, ...] (floats); stop_at: end
    early once r . r <= stop_at"""
    L0 = levels[0]
    dt, where = L0.dt, L0.where
    _sum = lambda t: t.dtype.type(np.sum(t, dtype=t.dtype))
    x, r, p, z, _, _ = setup(levels, x0, b0, sweeps, coarse_sweeps)
    rz = _sum((r[where] * z[where]).astype(dt))
    seq = [float(_sum((r * r).astype(dt)))]
    for _ in range(iters):
        if stop_at is not None and seq[-1] <= stop_at:
            break
        q = L0.A(p)
        pq = _sum((q[where] * p[where]).astype(dt))
        broken = rz == 0 or pq == 0
        alpha = dt(0) if broken else dt(rz / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        z = precondition(levels, r, sweeps, coarse_sweeps)
        rz_new = _sum((r[where] * z[where]).astype(dt))
        beta = dt(0) if broken else dt(rz_new / rz)
        p = (z + (beta * p).astype(dt)).astype(dt)
        rz = rz_new
        seq.append(float(_sum((r * r).astype(dt))))
    return seq


def replay(levels, x0, b0, rz0, trace, sweeps=2, coarse_sweeps=8):
    """mgcg_cases.replay on this module's preconditioner: the recurrences driven by the DEVICE's scalars (alpha_k = rz_k / pq_k,
    beta_k = rz_(k+1) / rz_k from rz_0 and the trace rows).  -> (x, r, p, z, checks, rr0, rz0); the levels' x_l, b_l are left
    in `levels`"""
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


def stage_applications(levels, sweeps, coarse_sweeps):
    """how many line stages (or point sweeps) one cycle applies over all levels"""
    total = 0
    for l, L in enumerate(levels):
        k = max(len(getattr(L, "stages", [])), 1)
        total += k * (coarse_sweeps if l == len(levels) - 1 else 2 * sweeps)
    return total
