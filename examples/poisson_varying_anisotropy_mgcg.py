#!/usr/bin/env python3
"""Conjugate gradients around a LINE-SMOOTHED V-cycle on the operator of poisson_varying_anisotropy_lines.py:
the symmetric flux form whose strong direction turns from dimension 1 to dimension 0 across the domain (a = eps^(1 - t),
c = eps^t, eps = 0.01), Omega = M^2, fully coarsened, coefficients injected, rscale = 4, omega = 0.8, 8 coarse sweeps.

Point Jacobi inside the preconditioner lets the iteration count grow with the anisotropy; alternating line stages (dim 0,
then dim 1) as plain cycles arrive in a handful of V(2,2) cycles; CG around ONE V(1,1) cycle of those stages arrives in about
as many iterations at half the smoothing.  The script solves to r . r <= 1e-16 r0 . r0 four ways and prints iterations /
cycles and wall time:

    multigrid.cg_solve(lines=True)   V(1,1) and V(2,2), alternating line stages
    multigrid.solve                  V(2,2), the same stages
    multigrid.cg_solve               V(2,2), point Jacobi

First, at Omega = 63^2, three iterations of cg_solve(lines=True) are checked BIT FOR BIT against the same recurrences in
NumPy -- one rounding per operation, the operators from the CPU oracle, alpha and beta from the device's traced scalars.

usage: examples/poisson_varying_anisotropy_mgcg.py [M]        (default 255; M = 2^k - 1)"""
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import poisson_varying_anisotropy_lines as ex  # noqa: E402  (puts the package and the oracle on sys.path)

RTOL2 = ex.RTOL2
COARSE_SWEEPS = ex.COARSE_SWEEPS
MAX_ITERS, MAX_CYCLES = ex.MAX_ITERS, ex.MAX_CYCLES


# ---------------------------------------------------------------- the same solver in NumPy, on the oracle's operators
def numpy_replay(texts, interiors, coefs, stages, b, rz0, trace, sweeps):
    """neptune_hip_mgcg_solve_lines as include/neptune_hip.h defines it, from x = 0, one rounding per operation (NumPy rounds
    every f64 operation once), driven by the device's scalars: alpha_k = rz_k / pq_k, beta_k = rz_(k+1) / rz_k; -> x"""
    import neptune_oracle as oracle
    mods = [oracle.Module.parse(t) for t in texts]
    where = [tuple(slice(lo, hi) for lo, hi in zip(*i)) for i in interiors]
    n = len(texts)
    xs = [np.zeros_like(a) for a, _ in coefs]
    rhs = [np.zeros_like(a) for a, _ in coefs]

    def A(l, v):
        out = np.zeros_like(v)
        mods[l].call("entry", out, v, *coefs[l])
        return out

    def stage(l, axis, lo, inv, up, first=False):
        """one line stage; first: without the apply, on q = +0 and x = +0 (d = b, x = (+0) + e)"""
        w = where[l]
        move = lambda f: np.moveaxis(f[w], axis, 0)
        d = move(rhs[l]) if first else move(rhs[l]) - move(A(l, xs[l]))
        lo, inv, up, x = move(lo), move(inv), move(up), move(xs[l])         # views: x is updated in place
        m = d.shape[0]
        g = [d[0] * inv[0]]
        for i in range(1, m):
            g.append((d[i] - lo[i] * g[i - 1]) * inv[i])
        e = g[m - 1]
        x[m - 1] = (0.0 if first else x[m - 1]) + e
        for i in range(m - 2, -1, -1):
            e = g[i] - up[i] * e
            x[i] = (0.0 if first else x[i]) + e

    def sweep(l, reverse=False):
        for st in (reversed(stages[l]) if reverse else stages[l]):
            stage(l, *st)

    def weigh(d, axis):
        k = d.shape[axis]
        t = lambda s: np.take(d, np.arange(s, k - 2 + s, 2), axis=axis)
        return (0.25 * t(0) + 0.5 * t(1)) + 0.25 * t(2)

    def interp(e, axis):
        m = e.shape[axis]
        pad = [(0, 0)] * e.ndim
        pad[axis] = (1, 1)
        p = np.pad(e, pad)
        shape = list(e.shape)
        shape[axis] = 2 * m + 1
        out = np.empty(shape)
        even, odd = [slice(None)] * e.ndim, [slice(None)] * e.ndim
        even[axis], odd[axis] = slice(0, None, 2), slice(1, None, 2)
        out[tuple(even)] = 0.5 * (np.take(p, np.arange(0, m + 1), axis=axis) + np.take(p, np.arange(1, m + 2), axis=axis))
        out[tuple(odd)] = e
        return out

    def cycle(l, pre):
        """Cycle(l) with `pre` pre-sweeps still to run (level 0 has run its first one already)"""
        if l == n - 1:
            for _ in range(COARSE_SWEEPS):
                sweep(l)
            return
        for _ in range(pre):
            sweep(l)
        t = rhs[l][where[l]] - A(l, xs[l])[where[l]]
        for axis in (1, 0):
            t = weigh(t, axis)
        rhs[l + 1][where[l + 1]] = 4.0 * t
        xs[l + 1][where[l + 1]] = 0.0
        cycle(l + 1, sweeps)
        e = xs[l + 1][where[l + 1]]
        for axis in (1, 0):
            e = interp(e, axis)
        xs[l][where[l]] = xs[l][where[l]] + e
        for _ in range(sweeps):
            sweep(l, reverse=True)

    def precondition(r):
        """z = M(r): the cycle on A z = r from z = 0, its first stage apply-free"""
        rhs[0] = r
        xs[0] = np.zeros_like(r)
        stage(0, *stages[0][0], first=True)
        for st in stages[0][1:]:
            stage(0, *st)
        cycle(0, sweeps - 1)
        return xs[0].copy()

    w0 = where[0]
    x = np.zeros_like(b)
    r = np.zeros_like(b)
    r[w0] = b[w0] - A(0, x)[w0]
    z = precondition(r)
    p = z.copy()
    rz = rz0
    for pq, rz_new, _ in trace:
        q = np.zeros_like(p)
        q[w0] = A(0, p)[w0]
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = precondition(r)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 255
    import torch
    from neptune_hip import fields, multigrid
    F = fields.DeviceField

    # 1. Omega = 63^2: x after three iterations of V(1,1) against the NumPy replay, bit for bit
    h, texts, interiors, coefs, stages = ex.hierarchy(63, True)
    b = ex.right_hand_side(63)
    x = F.from_numpy(np.zeros_like(b))
    iters, rr0, rr_last, trace = multigrid.cg_solve(h, x, F.from_numpy(b), sweeps=1, coarse_sweeps=COARSE_SWEEPS, max_iters=3, trace=True,
                                                    lines=True)
    want = numpy_replay(texts, interiors, coefs, stages, b, multigrid.cg_rz0(), trace, 1)
    got = x.numpy()
    ok = iters == 3 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    print(f"63^2, {len(h)} levels, CG around V(1,1) with alternating line stages, {iters} iterations: r.r {rr0:.3e} -> {rr_last:.3e}, launches "
          f"(plain, graph, fallback, checks) = {multigrid.cg_counts()}, x bit for bit as the NumPy replay on the oracle: {ok}")

    # 2. the size asked for: four solvers to the same r . r
    b = ex.right_hand_side(m)
    bf = F.from_numpy(b)
    hs = {"lines": ex.hierarchy(m, True)[0], "point": ex.hierarchy(m, False)[0]}
    _, rr0, _ = multigrid.cg_solve(hs["point"], F.from_numpy(np.zeros_like(b)), bf, max_iters=0)
    tol2 = RTOL2 * rr0
    runs = [("cg_solve(lines=True) V(1,1), line stages", "lines", "cg", 1), ("cg_solve(lines=True) V(2,2), line stages", "lines", "cg", 2),
            ("solve V(2,2), line stages", "lines", "solve", 2), ("cg_solve V(2,2), point Jacobi", "point", "cg", 2)]
    results = {}
    for label, name, solver, sweeps in runs:
        for warm in (True, False):                    # the first solve pays first-use tuning and workspace growth
            x = F.from_numpy(np.zeros_like(b))
            work = [F.empty_like(x) for _ in range(3)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if solver == "solve":
                steps, _, rr, _ = multigrid.solve(hs[name], x, bf, pre=sweeps, post=sweeps, coarse_sweeps=COARSE_SWEEPS, max_cycles=MAX_CYCLES,
                                                  tol2=tol2)
            else:
                steps, _, rr = multigrid.cg_solve(hs[name], x, bf, sweeps=sweeps, coarse_sweeps=COARSE_SWEEPS, max_iters=MAX_ITERS, tol2=tol2,
                                                  work=work, lines=name == "lines")
            seconds = time.perf_counter() - t0
        results[label] = (steps, rr, seconds, x.numpy(), "cycles" if solver == "solve" else "iterations")
    print(f"{m}^2, eps = {ex.EPS}, the strong direction turning from dim 1 to dim 0 across the domain, omega = {ex.OMEGA}, to r.r <= {RTOL2:g} "
          f"r0.r0 ({len(hs['lines'])} levels):")
    for label, (steps, rr, seconds, _, unit) in results.items():
        reached = "reached" if rr <= tol2 else f"NOT reached: r.r / r0.r0 = {rr / rr0:.1e}"
        print(f"  multigrid.{label:<44}: {steps} {unit}, {seconds * 1e3:.1f} ms ({reached})")
    ref = results[runs[3][0]][3]
    print(f"  max |u_lines_cg - u_point_cg| = {float(np.max(np.abs(results[runs[0][0]][3] - ref))):.2e}")
    ok = ok and all(r[1] <= tol2 for r in results.values())
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
