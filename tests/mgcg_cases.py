"""The NumPy restatement of multigrid-preconditioned conjugate gradients (neptune_hip_mgcg_solve), on the
kernels' restatement of mg_cases (smooth, restrict, prolong_add, Level, Operator) and the trace-replay pattern of pcg_cases.

Everything follows the normative definition in include/neptune_hip.h: arithmetic in the element type with one `.astype(dt)`
per operation, the operator itself from the oracle.  The preconditioner z = M(r) is one V(sweeps, sweeps) cycle on A z = r
from z = 0 whose first pre-sweep on level 0 is z = minv_0 * r on EVERY cell of the box (minv_0 is +0 outside Omega) and whose
last post-sweep also yields r . z over Omega.  The sums (pq, rz, rr) are compared as exact sums of the restatement's own
terms with the bound 2 (n - 1) eps sum |t_i| two summation orders may differ by; the fields, driven by the device's traced
scalars, bit for bit."""
import numpy as np

import cg_cases as cc
import mg_cases as mgc
import monitor_cases as mc

expected_stop = cc.expected_stop        # what the loop's definition gives on an r . r sequence: (iters_done, checks)
tol_between = mgc.tol_between           # a threshold between two check values a factor >= 4 apart


# ---------------------------------------------------------------- the anisotropic star
def aniso_module(shape, weights, dtype=np.float64, bounds=None):
    """NeptuneIR text of @entry(out, in): out<p> = (2 * sum of weights) * u<p> - sum over axes d of weights[d] * (u<p - e_d> +
    u<p + e_d>) one cell in from every face, copy-through on the rim: the unscaled operator -sum_d weights[d] u_dd, with
    its own side weight per axis (mg_cases.mg_module is weights = 1 everywhere, in another order of additions).
    bounds: (lb, ub) of the apply instead of one cell in from every face"""
    rank = len(shape)
    assert len(weights) == rank
    if bounds is None:
        bounds = ([1] * rank, [n - 1 for n in shape])
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "x".join(["?"] * rank) + "x" + elem
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    zero = [0] * rank
    body = [f"        %c = neptune_ir.access %a[{lst(zero)}] : !temp -> {elem}",
            f"        %wc = arith.constant {float(2.0 * sum(float(w) for w in weights))!r} : {elem}",
            f"        %acc0 = arith.mulf %wc, %c : {elem}"]
    for d in range(rank):
        lo, hi = list(zero), list(zero)
        lo[d], hi[d] = -1, 1
        body += [f"        %m{d} = neptune_ir.access %a[{lst(lo)}] : !temp -> {elem}",
                 f"        %p{d} = neptune_ir.access %a[{lst(hi)}] : !temp -> {elem}",
                 f"        %s{d} = arith.addf %m{d}, %p{d} : {elem}",
                 f"        %w{d} = arith.constant {-float(weights[d])!r} : {elem}",
                 f"        %t{d} = arith.mulf %w{d}, %s{d} : {elem}",
                 f"        %acc{d + 1} = arith.addf %acc{d}, %t{d} : {elem}"]
    body.append(f"        neptune_ir.yield %acc{rank} : {elem}")
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(zero)}], ub = [{lst(shape)}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst(bounds[0])}], ub = [{lst(bounds[1])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu   = neptune_ir.wrap %in : memref<{mr}> -> !field",
           "    %u    = neptune_ir.load %fu : !field -> !temp",
           "    %r = neptune_ir.apply(%u) attributes {bounds = #bi} : (!temp) -> !temp {",
           f"      ^bb0({idx}, %a: !temp):"] + body + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def aniso_levels(omega, n_levels, weights, damp, dtype=np.float64, minv_outside=0.0):
    """restatement levels of the anisotropic star on whole-interior boxes (rim of one cell), damped-Jacobi weights
    damp / diagonal on Omega and `minv_outside` elsewhere; -> (levels, module texts)"""
    dt = np.dtype(dtype).type
    shapes = mgc.level_shapes(omega, n_levels)
    texts = [aniso_module(shape, weights, dtype) for shape, _ in shapes]
    levels = []
    for text, (shape, where) in zip(texts, shapes):
        minv = np.full(shape, minv_outside, dtype)
        minv[where] = dt(dt(damp) / dt(2.0 * sum(float(w) for w in weights)))
        levels.append(mgc.Level(mgc.Operator(text), shape, where, minv, dtype))
    return levels, texts


# ---------------------------------------------------------------- the preconditioner
def start(levels, work_fill=np.nan):
    """the state the set-up leaves before the first cycle: the coarser x zero-filled (whole box), the coarser b and every q
    holding `work_fill` (what the device's work fields hold before the call)"""
    for l, L in enumerate(levels):
        if l > 0:
            L.x = np.zeros(L.shape, L.dt)
            L.b = np.full(L.shape, work_fill, L.dt)
        L.q = np.full(L.shape, work_fill, L.dt)


def first_sweep(levels, r):
    """the cycle's first pre-sweep on level 0, from z = 0 with A(0) = 0: z = minv_0 * r on every cell, one rounding"""
    L0 = levels[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return (L0.minv * r).astype(L0.dt)


def rest_of_cycle(levels, r, z, sweeps, coarse_sweeps):
    """everything of M after its first pre-sweep: level 0 carries (z, r) for (x, b); -> z = M(r), the levels' fields left as
    the device leaves them"""
    L0, L1 = levels[0], levels[1]
    L0.x, L0.b = z, r
    for _ in range(sweeps - 1):
        mgc.sweep(L0)
    L0.q = L0.A(L0.x)
    L1.b, L1.x = mgc.restrict(L0.b, L0.q, L0.where, L0.rscale, L1.b, L1.x, L1.where)
    mgc.cycle(levels, 1, sweeps, sweeps, coarse_sweeps)
    L0.x = mgc.prolong_add(L1.x, L1.where, L0.x, L0.where)
    for _ in range(sweeps):
        mgc.sweep(L0)
    return L0.x


def precondition(levels, r, sweeps=2, coarse_sweeps=8):
    """z = M(r): one V(sweeps, sweeps) cycle of the definition on A_0 z = r from z = 0 (call start(levels) once before)"""
    assert len(levels) >= 2 and sweeps >= 1
    return rest_of_cycle(levels, r, first_sweep(levels, r), sweeps, coarse_sweeps)


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


def _sum(terms: np.ndarray):
    return terms.dtype.type(np.sum(terms, dtype=terms.dtype))


def numpy_mgcg(levels, x0, b0, iters, sweeps=2, coarse_sweeps=8, stop_at=None):
    """the recurrences of the definition with numpy's own sums: -> the r . r sequence [rr_0, rr_1, ...] (floats), for the stop
    tests and the convergence checks; stop_at: end early once r . r <= stop_at"""
    L0 = levels[0]
    dt, where = L0.dt, L0.where
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
    """The definition's recurrences driven by the DEVICE's scalars: iteration k takes alpha_k = rz_k / pq_k and
    beta_k = rz_(k+1) / rz_k from rz_0 and the trace rows (pq_k, rz_(k+1), rr_(k+1)), each one division in the element type,
    and q from the oracle's operator.  -> (x, r, p, z, checks, rr0, rz0): checks[k] = the (terms' sum, bound) pairs of pq, rz'
    and rr' of the replay's own fields, rr0 / rz0 those of the set-up; the levels' x_l, b_l are left in `levels` (level 0's
    are z and r)."""
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


def star_levels(omega, n_levels, dtype, damp, texts=None):
    """mg_cases.star_levels with the weights this solver needs: level 0's minv is +0 outside Omega (the definition forms
    z = minv_0 * r on the whole box), the coarser levels' stay NaN there (never read); -> (levels, module texts)"""
    levels, texts = mgc.star_levels(omega, n_levels, dtype, damp, texts=texts)
    L0 = levels[0]
    L0.minv = mgc.minv_field(L0.shape, L0.where, dtype, damp, outside=0.0)
    return levels, texts
