#!/usr/bin/env python3
"""An anisotropic 3-D operator, one weak axis, solved three ways on the device:

    (2 eps + 4) u - eps (u<-1,0,0> + u<+1,0,0>) - (the four neighbours along the other two axes) = b
    on the interior Omega = M^3, u = 0 on the rim; eps = 0.03

Point-Jacobi smoothing with full coarsening cannot smooth the error along the weak axis, so plain V-cycles
(multigrid.solve) stall; plain conjugate gradients (apply.cg_solve) need an iteration count that
grows with M.  Conjugate gradients wrapped around ONE symmetric V-cycle (multigrid.cg_solve, neptune_hip_mgcg_solve,
DESIGN 3.15) keep the grid-independent count and repair the stall.

The script solves to r . r <= 1e-16 r0 . r0 with all three and prints iterations / cycles, finest-field passes (counts, not
timings) and wall time.  First, at Omega = 31^3 (five levels), multigrid.cg_solve is checked BIT FOR BIT against the same
driver in NumPy -- one rounding per operation, the operator from the CPU oracle, the recurrences driven by the device's
traced scalars: whatever order the device summed in, the fields it holds are then fully determined.

usage: examples/poisson_anisotropic_mgcg.py [M]        (default 127: Omega = 127^3, seven levels; M = 2^k - 1)"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

EPS = 0.03
RTOL2 = 1e-16
SWEEPS, COARSE_SWEEPS = 2, 8
OMEGA = 0.8
DIAGONAL = 2.0 * EPS + 4.0
MAX_ITERS, MAX_CYCLES, MAX_CG_ITERS, CHECK_EVERY_CG = 200, 400, 6000, 10


def build_text(m):
    """@entry(out, u): out = A(u) as above on the interior m^3 of a box (m + 2)^3, copy-through on the rim"""
    import neptune as nep
    nep.reset()
    n = m + 2
    box = ([0, 0, 0], [n, n, n])
    interior = ([1, 1, 1], [n - 1, n - 1, n - 1])
    c = nep.get_compiler()
    c.start_function("entry", [("memref", 3), ("memref", 3)])
    fout = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    u = nep.load(nep.wrap(nep.Expr(c.get_function_arg(1)), box))

    @nep.apply(inputs=[u], bounds=interior)
    def aniso(x):
        return x[0, 0, 0] * DIAGONAL - ((x[-1, 0, 0] + x[1, 0, 0]) * EPS + (x[0, -1, 0] + x[0, 1, 0] + x[0, 0, -1] + x[0, 0, 1]))

    nep.store(aniso, fout)
    c.create_return(nep.unwrap(fout)._handle)
    c.end_function()
    text = c.dump()
    nep.reset()
    return text, interior


def level_extents(m):
    """m, (m - 1) / 2, ... down to 1 (or to the first even extent)"""
    out = [m]
    while out[-1] >= 3 and out[-1] % 2 == 1:
        out.append((out[-1] - 1) // 2)
    return out


def right_hand_side(m):
    rng = np.random.default_rng(11)
    b = np.zeros((m + 2,) * 3)
    b[1:-1, 1:-1, 1:-1] = rng.standard_normal((m,) * 3)
    return b


def passes_per_cycle(n_levels, pre, post, rank=3):
    """finest-field passes of one V(pre, post) cycle: 7 per sweep (apply 2, smoother 5), apply + restriction, prolongation"""
    total = 0.0
    for l in range(n_levels):
        size = 1.0 / (2 ** rank) ** l
        if l == n_levels - 1:
            total += size * 7 * COARSE_SWEEPS
        else:
            total += size * (7 * (pre + post) + 2 + (2 + 2 / 2 ** rank) + (2 + 1 / 2 ** rank))
    return total


def passes_per_iteration(n_levels):
    """the dot-monitored apply 2, the update 8 (it stores z = minv r: the cycle's first sweep), the cycle without that sweep,
    the direction 3"""
    return 2 + 8 + (passes_per_cycle(n_levels, SWEEPS, SWEEPS) - 7) + 3


# ---------------------------------------------------------------- the same driver in NumPy, on the oracle's operator
def numpy_replay(texts, interiors, minvs, b, rz0, trace):
    """neptune_hip_mgcg_solve as include/neptune_hip.h defines it, one rounding per operation, from x = 0, with alpha_k =
    rz_k / pq_k and beta_k = rz_(k+1) / rz_k taken from the device's rz_0 and trace rows (pq_k, rz_(k+1), rr_(k+1)); -> x"""
    import neptune_oracle as oracle
    mods = [oracle.Module.parse(t) for t in texts]
    where = [tuple(slice(lo, hi) for lo, hi in zip(*i)) for i in interiors]
    n = len(texts)
    xs = [np.zeros_like(m) for m in minvs]
    rhs = [None] + [np.zeros_like(m) for m in minvs[1:]]

    def A(l, v):
        out = np.zeros_like(v)
        mods[l].call("entry", out, v)
        return out

    def sweep(l):
        w = where[l]
        d = rhs[l][w] - A(l, xs[l])[w]
        xs[l][w] = xs[l][w] + minvs[l][w] * d

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

    def cycle(l, first_sweep_done=False):
        if l == n - 1:
            for _ in range(COARSE_SWEEPS):
                sweep(l)
            return
        for _ in range(SWEEPS - 1 if first_sweep_done else SWEEPS):
            sweep(l)
        t = rhs[l][where[l]] - A(l, xs[l])[where[l]]
        for axis in (2, 1, 0):
            t = weigh(t, axis)
        rhs[l + 1][where[l + 1]] = 4.0 * t
        xs[l + 1][where[l + 1]] = 0.0
        cycle(l + 1)
        e = xs[l + 1][where[l + 1]]
        for axis in (2, 1, 0):
            e = interp(e, axis)
        xs[l][where[l]] = xs[l][where[l]] + e
        for _ in range(SWEEPS):
            sweep(l)

    def precondition(r):
        """z = M(r): the first pre-sweep of level 0 is z = minv r on the whole box (from z = 0, A(0) = 0)"""
        rhs[0] = r
        xs[0] = minvs[0] * r
        cycle(0, first_sweep_done=True)
        return xs[0].copy()

    x = np.zeros_like(b)
    r = np.zeros_like(b)
    r[where[0]] = b[where[0]] - A(0, x)[where[0]]
    z = precondition(r)
    p = z.copy()
    rz = np.float64(rz0)
    for pq, rz_new, _ in trace:
        q = A(0, p)
        broken = rz == 0 or pq == 0
        alpha = np.float64(0) if broken else rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = precondition(r)
        beta = np.float64(0) if broken else rz_new / rz
        p = z + beta * p
        rz = rz_new
    return x


# ---------------------------------------------------------------- the device
def hierarchy(m):
    """-> (multigrid.Hierarchy, level-0 interior, module texts, interiors, minv arrays)"""
    from neptune_hip import fields, lowering, multigrid
    F = fields.DeviceField
    levels, texts, interiors, minvs = [], [], [], []
    for l, ml in enumerate(level_extents(m)):
        text, interior = build_text(ml)
        mod = lowering.compile_module(text, dot_entries=(l == 0))
        entry = mod.dot_entry("entry") if l == 0 else mod.geom_entry("entry")
        like = F.from_numpy(np.zeros((ml + 2,) * 3))
        minv = multigrid.jacobi_weights(entry, like, interior, omega=OMEGA)      # omega / diagonal on Omega, +0 outside
        levels.append(multigrid.Level(entry, like, interior, minv=minv, rscale=4.0))
        texts.append(text)
        interiors.append(interior)
        minvs.append(minv.numpy())
    return multigrid.Hierarchy(levels), interiors[0], texts, interiors, minvs


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 127
    import torch
    from neptune_hip import apply, fields, multigrid
    F = fields.DeviceField

    # 1. Omega = 31^3, five levels: the device's x against the NumPy driver on the oracle, bit for bit
    h, _, texts, interiors, minvs = hierarchy(31)
    b = right_hand_side(31)
    x = F.from_numpy(np.zeros_like(b))
    iters, rr0, rr_last, trace = multigrid.cg_solve(h, x, F.from_numpy(b), sweeps=SWEEPS, coarse_sweeps=COARSE_SWEEPS, max_iters=6,
                                                    trace=True)
    want = numpy_replay(texts, interiors, minvs, b, multigrid.cg_rz0(), trace)
    got = x.numpy()
    ok = len(h) == 5 and iters == 6 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    print(f"31^3, {len(h)} levels, {iters} iterations: r.r {rr0:.3e} -> {rr_last:.3e}, launches (plain, graph, fallback, checks) = "
          f"{multigrid.cg_counts()}, x bit for bit as the NumPy driver on the oracle: {ok}")

    # 2. the size asked for: three solvers to the same r . r
    h, interior, _, _, _ = hierarchy(m)
    entry = h.levels[0].entry
    b = right_hand_side(m)
    bf = F.from_numpy(b)
    n_levels = len(h)
    for warm in (True, False):                    # the first solve pays first-use tuning and workspace growth
        x1 = F.from_numpy(np.zeros_like(b))
        _, rr0, _ = multigrid.cg_solve(h, x1, bf, max_iters=0)
        work = [F.empty_like(x1) for _ in range(3)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it1, _, rr1 = multigrid.cg_solve(h, x1, bf, sweeps=SWEEPS, coarse_sweeps=COARSE_SWEEPS, max_iters=MAX_ITERS, tol2=RTOL2 * rr0,
                                         work=work)
        t1 = time.perf_counter() - t0
        x2 = F.from_numpy(np.zeros_like(b))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it2, _, rr2, _ = multigrid.solve(h, x2, bf, pre=SWEEPS, post=SWEEPS, coarse_sweeps=COARSE_SWEEPS, max_cycles=MAX_CYCLES,
                                         tol2=RTOL2 * rr0, check_every=4)
        t2 = time.perf_counter() - t0
        x3 = F.from_numpy(np.zeros_like(b))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it3, _, rr3 = apply.cg_solve(entry, x3, bf, interior, MAX_CG_ITERS, RTOL2 * rr0, check_every=CHECK_EVERY_CG, work=work)
        t3 = time.perf_counter() - t0
    ok = ok and rr1 <= RTOL2 * rr0 and rr3 <= RTOL2 * rr0
    per_it, per_cycle = passes_per_iteration(n_levels), passes_per_cycle(n_levels, SWEEPS, SWEEPS)
    reached = "reached" if rr2 <= RTOL2 * rr0 else f"NOT reached: r.r / r0.r0 = {rr2 / rr0:.1e}"
    print(f"{m}^3, {n_levels} levels, eps = {EPS}, to r.r <= {RTOL2:g} r0.r0:")
    print(f"  multigrid.cg_solve V({SWEEPS},{SWEEPS}): {it1} iterations x {per_it:.1f} passes = {it1 * per_it:.0f} passes, {t1 * 1e3:.1f} ms")
    print(f"  multigrid.solve V({SWEEPS},{SWEEPS}): {it2} cycles x {per_cycle:.1f} passes = {it2 * per_cycle:.0f} passes (+ 4 per check), "
          f"{t2 * 1e3:.1f} ms ({reached})")
    print(f"  apply.cg_solve: {it3} iterations x 11 passes = {it3 * 11} passes, {t3 * 1e3:.1f} ms")
    print(f"  max |u_mgcg - u_cg| = {float(np.max(np.abs(x1.numpy() - x3.numpy()))):.2e}")
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
