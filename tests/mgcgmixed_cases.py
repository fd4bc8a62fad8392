"""The NumPy restatement of mixed-precision multigrid-preconditioned conjugate gradients (neptune_hip_mgcg_solve_mixed,
DESIGN 3.19), on the restatements of mg_cases and mgcg_cases.

Everything follows the normative definition in include/neptune_hip.h.  The outer recurrences (x, r, p, q and the scalars)
are np.float64, the outer operator comes from the oracle at f64; the levels of the preconditioner are np.float32 levels of
mg_cases (their operators from the oracle at f32) and run the existing restatement of the cycle unchanged.  One `.astype` per operation;
narrow is `.astype(np.float32)`, widen is `.astype(np.float64)`.

The sums are compared as cg_cases.dot_terms does: the exact sum (math.fsum) of the restatement's own f64 terms with the
bound 2 (n - 1) eps64 sum |t_i| that two summation orders may differ by.  For r . z the terms are widen(r32) * widen(z32): the
product of two f32 values is exact in f64.  The fields, driven by the device's traced scalars, are compared bit for bit."""
import math

import numpy as np

import cg_cases as cc
import mg_cases as mgc
import mgcg_cases as mg
import mgcglines_cases as mlc

D, S = np.float64, np.float32
expected_stop = mg.expected_stop
tol_between = mg.tol_between


def narrow(a: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return a.astype(S)


def widen(a: np.ndarray) -> np.ndarray:
    return a.astype(D)


def wide_dot_terms(a32: np.ndarray, b32: np.ndarray, where):
    """-> (sum, bound) of the terms widen(a32) * widen(b32) over `where`: each term exact in f64, summed exactly; bound =
    2 (n - 1) eps64 sum |t_i|"""
    assert a32.dtype == S and b32.dtype == S
    return cc.dot_terms(widen(a32), widen(b32), where)


class Problem:
    """an outer f64 operator (a callable u -> A(u) on f64 arrays) and f32 levels of mg_cases whose level 0 has the outer
    operator's box and Omega"""

    def __init__(self, outer_A, levels):
        assert all(L.dt is S for L in levels) and len(levels) >= 2
        self.A, self.levels = outer_A, levels
        self.shape, self.where = levels[0].shape, levels[0].where


def star_problem(omega, n_levels, damp, texts64=None, texts32=None):
    """the unscaled Poisson star: outer operator lowered at f64, the levels' at f32; level 0's minv +0 outside Omega;
    -> (Problem, level 0's f64 module text, the f32 module texts)"""
    levels, texts32 = mg.star_levels(omega, n_levels, S, damp, texts=texts32)
    text64 = texts64 or mgc.mg_module(levels[0].shape, D)
    return Problem(mgc.Operator(text64), levels), text64, texts32


def aniso_problem(omega, n_levels, weights, damp):
    """mgcg_cases' anisotropic star -sum_d weights[d] u_dd, outer at f64 and levels at f32"""
    levels, texts32 = mg.aniso_levels(omega, n_levels, weights, damp, dtype=S)
    text64 = mg.aniso_module(levels[0].shape, weights, D)
    return Problem(mgc.Operator(text64), levels), text64, texts32


# ---------------------------------------------------------------- the definition, step by step
def store_residual(P: Problem, x0, b0):
    """steps 1 and 2 of the set-up: -> (x, r, r32, z32, rr0 as (terms' sum, bound)); what a call that runs no iteration
    leaves behind"""
    L0 = P.levels[0]
    mg.start(P.levels)
    x = x0.copy()
    q = P.A(x)
    r = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r[P.where] = (b0[P.where] - q[P.where]).astype(D)
    rr0 = cc.dot_terms(r, r, P.where)
    r32 = narrow(r)
    z32 = np.zeros(P.shape, S)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        z32[P.where] = (L0.minv[P.where] * r32[P.where]).astype(S)
    return x, r, r32, z32, rr0


def precondition_stored(P: Problem, r32, z32, sweeps, coarse_sweeps):
    """the rest of M32 on (z32, r32): -> z32 = M32(r32), the levels' fields left as the device leaves them.  The cycle is
    mgcglines_cases.rest_of_cycle: mgcg_cases' own for plain levels, and it honours `axes` (semi-coarsening) and `stages`
    (line stages; level 0 has none here) where the levels carry them"""
    L0 = P.levels[0]
    assert not getattr(L0, "stages", [])
    L0.x, L0.b = z32, r32
    return mlc.rest_of_cycle(P.levels, sweeps, coarse_sweeps)


def update(P: Problem, alpha, x, r, p, q):
    """step 2 of the iteration on all cells: -> (x, r, r32, z32 after the first pre-sweep)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        x = (x + (alpha * p).astype(D)).astype(D)
        r = (r - (alpha * q).astype(D)).astype(D)
        r32 = narrow(r)
        z32 = (P.levels[0].minv * r32).astype(S)
    return x, r, r32, z32


def setup(P: Problem, x0, b0, sweeps=2, coarse_sweeps=8):
    """the definition's set-up: -> (x, r, p, r32, z32, rr0 as (terms' sum, bound), rz0 likewise)"""
    x, r, r32, z32, rr0 = store_residual(P, x0, b0)
    z32 = precondition_stored(P, r32, z32, sweeps, coarse_sweeps)
    rz0 = wide_dot_terms(r32, z32, P.where)
    return x, r, widen(z32), r32, z32, rr0, rz0


def _sum(terms: np.ndarray):
    return D(np.sum(terms, dtype=D))


def numpy_mgcg_mixed(P: Problem, x0, b0, iters, sweeps=2, coarse_sweeps=8, stop_at=None):
    """the recurrences of the definition with numpy's own sums: -> ([rr_0, rr_1, ...] as floats, x); stop_at: end early once
    r . r <= stop_at"""
    where = P.where
    x, r, p, r32, z32, _, _ = setup(P, x0, b0, sweeps, coarse_sweeps)
    rz = _sum(widen(r32[where]) * widen(z32[where]))
    seq = [float(_sum((r * r).astype(D)))]
    for _ in range(iters):
        if stop_at is not None and seq[-1] <= stop_at:
            break
        q = P.A(p)
        pq = _sum((q[where] * p[where]).astype(D))
        broken = rz == 0 or pq == 0
        alpha = D(0) if broken else D(rz / pq)
        x, r, r32, z32 = update(P, alpha, x, r, p, q)
        z32 = precondition_stored(P, r32, z32, sweeps, coarse_sweeps)
        rz_new = _sum(widen(r32[where]) * widen(z32[where]))
        beta = D(0) if broken else D(rz_new / rz)
        p = (widen(z32) + (beta * p).astype(D)).astype(D)
        rz = rz_new
        seq.append(float(_sum((r * r).astype(D))))
    return seq, x


def replay(P: Problem, x0, b0, rz0, trace, sweeps=2, coarse_sweeps=8):
    """The definition's recurrences driven by the DEVICE's scalars, as mgcg_cases.replay: iteration k takes alpha_k =
    rz_k / pq_k and beta_k = rz_(k+1) / rz_k from rz_0 and the trace rows (pq_k, rz_(k+1), rr_(k+1)), each one division in
    f64, and q from the oracle's f64 operator.  -> (x, r, p, r32, z32, checks, rr0, rz0): checks[k] = the (terms' sum, bound)
    pairs of pq, rz' and rr' of the replay's own fields; the levels' x_l, b_l are left in P.levels (level 0's are z32, r32)."""
    where = P.where
    x, r, p, r32, z32, rr0, rz0_ref = setup(P, x0, b0, sweeps, coarse_sweeps)
    rz = D(rz0)
    checks = []
    everywhere = tuple(slice(None) for _ in x.shape)
    for k in range(len(trace)):
        pq, rz_new = D(trace[k][0]), D(trace[k][1])
        q = P.A(p)
        pq_ref = cc.dot_terms(q, p, where)
        broken = rz == 0 or pq == 0
        alpha = D(0) if broken else D(rz / pq)
        x, r, r32, z32 = update(P, alpha, x, r, p, q)
        rr_ref = cc.dot_terms(r, r, everywhere)
        z32 = precondition_stored(P, r32, z32, sweeps, coarse_sweeps)
        checks.append((pq_ref, wide_dot_terms(r32, z32, where), rr_ref))
        beta = D(0) if broken else D(rz_new / rz)
        p = (widen(z32) + (beta * p).astype(D)).astype(D)
        rz = rz_new
    return x, r, p, r32, z32, checks, rr0, rz0_ref


def true_residual(P: Problem, x, b0) -> float:
    """sum over Omega of (b - A(x))^2 in f64 by the oracle, the terms summed exactly"""
    q = P.A(x)
    d = (b0[P.where] - q[P.where]).astype(D)
    return math.fsum(float(v) * float(v) for v in d.ravel())


# ---------------------------------------------------------------- the device side of a Problem (GPU tests)
class Device:
    """what a GPU test hands to multigrid.cg_solve_mixed: outer (an f64 Level), h (the f32 Hierarchy, h.x[0] = z32 and
    h.b[0] = r32), x, b and work = [r, p, q]"""


def _bounds(where):
    return [s.start for s in where], [s.stop for s in where]


def device_problem(nh, P: Problem, entry64, entries32, x0, b0, others64=(), others32=None, offset=0) -> Device:
    """P on the device.  Every work field (r, p, q, r32, z32, q_l, and x_l, b_l for l >= 1) holds NaN before the call.
    offset: the fields the flat kernels stream (x, b, r, p, q, r32, z32, level 0's minv and q) start that many ELEMENTS into
    larger allocations -- 8 bytes for an f64 field, 4 for an f32 one with offset = 1: not 16-byte aligned.  A restatement
    level with `stages` gets them as line stages."""
    import solver_trace_cases as stc
    F = nh.fields.DeviceField
    make = (lambda a: stc.offset_field(nh, a, offset)) if offset else F.from_numpy
    nan = lambda shape, dt: np.full(shape, np.nan, dt)
    dev = Device()
    dev.outer = nh.mg.Level(entry64, F.from_numpy(np.zeros(P.shape, D)), _bounds(P.where), others=list(others64))
    levels = []
    for l, R in enumerate(P.levels):
        lines = [nh.mg.LineStage(ax, F.from_numpy(lo), F.from_numpy(inv), F.from_numpy(up)) for ax, lo, inv, up in getattr(R, "stages", [])]
        minv = make(R.minv) if l == 0 else F.from_numpy(R.minv)
        levels.append(nh.mg.Level(entries32[l], F.from_numpy(np.zeros(R.shape, S)), _bounds(R.where),
                                  others=list(others32[l]) if others32 else [], minv=minv, rscale=R.rscale, lines=lines))
    h = nh.mg.Hierarchy(levels)
    h.q = [make(nan(f.shape, S)) if l == 0 else F.from_numpy(nan(f.shape, S)) for l, f in enumerate(h.q)]
    h.x = [make(nan(P.shape, S))] + [F.from_numpy(nan(f.shape, S)) for f in h.x[1:]]
    h.b = [make(nan(P.shape, S))] + [F.from_numpy(nan(f.shape, S)) for f in h.b[1:]]
    dev.h, dev.x, dev.b = h, make(x0), make(b0)
    dev.work = [make(nan(P.shape, D)) for _ in range(3)]
    return dev
