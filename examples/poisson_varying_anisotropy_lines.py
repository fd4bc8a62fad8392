#!/usr/bin/env python3
"""An anisotropic 2-D operator whose strong direction CHANGES across the domain, repaired by line smoothers:

    A(u)_p = 1/2 (a_p + a_(p-e0)) (u_p - u_(p-e0)) + 1/2 (a_p + a_(p+e0)) (u_p - u_(p+e0))
           + 1/2 (c_p + c_(p-e1)) (u_p - u_(p-e1)) + 1/2 (c_p + c_(p+e1)) (u_p - u_(p+e1))      (symmetric flux form)
    on the interior Omega = M^2 of an (M + 2)^2 box, u = 0 on the rim; cell fields a = eps^(1 - t), c = eps^t with
    t = j / (M + 1) for column j and eps = 0.01: dimension 1 is strong on the left, dimension 0 on the right

Point Jacobi smooths along the locally strong dimension only and semi-coarsening has no single choice of kept axes that is
right everywhere.  A line stage solves the operator's tridiagonal part along one dimension exactly; a dim-0 stage followed
by a dim-1 stage in every sweep smooths whatever the local direction is.  The hierarchy is fully coarsened, the coefficients
are injected to the coarser levels (a[0::2, 0::2] on the box), rscale = 4.

The script solves to r . r <= 1e-16 r0 . r0 three ways and prints cycles / iterations and wall time:

    multigrid.solve     with alternating line stages (multigrid.line_weights along dim 0, then dim 1)
    multigrid.solve     with point Jacobi
    multigrid.cg_solve  with point Jacobi

First, at Omega = 63^2, multigrid.solve with alternating stages is checked BIT FOR BIT against the same driver in NumPy --
one rounding per operation, the operators from the CPU oracle.

usage: examples/poisson_varying_anisotropy_lines.py [M]        (default 255; M = 2^k - 1)"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

EPS = 0.01
RTOL2 = 1e-16
SWEEPS, COARSE_SWEEPS = 2, 8
OMEGA = 0.8
MAX_ITERS, MAX_CYCLES = 400, 100


def build_text(n):
    """@entry(out, u, a, c): the flux-form operator on the interior of an n x n box, copy-through on the rim"""
    import neptune as nep
    nep.reset()
    box = ([0, 0], [n, n])
    interior = ([1, 1], [n - 1, n - 1])
    k = nep.get_compiler()
    k.start_function("entry", [("memref", 2)] * 4)
    fout = nep.wrap(nep.Expr(k.get_function_arg(0)), box)
    u, a, c = (nep.load(nep.wrap(nep.Expr(k.get_function_arg(i)), box)) for i in (1, 2, 3))

    @nep.apply(inputs=[u, a, c], bounds=interior)
    def flux(x, ka, kc):
        return ((((ka[0, 0] + ka[-1, 0]) * 0.5) * (x[0, 0] - x[-1, 0]) + ((ka[0, 0] + ka[1, 0]) * 0.5) * (x[0, 0] - x[1, 0]))
                + ((kc[0, 0] + kc[0, -1]) * 0.5) * (x[0, 0] - x[0, -1])) + ((kc[0, 0] + kc[0, 1]) * 0.5) * (x[0, 0] - x[0, 1])

    nep.store(flux, fout)
    k.create_return(nep.unwrap(fout)._handle)
    k.end_function()
    text = k.dump()
    nep.reset()
    return text, interior


def coefficients(m):
    """per level (a, c) over the box, finest first: the fields above on the (m + 2)^2 box, injected down to the 3 x 3 box"""
    n = m + 2
    t = np.arange(n) / (n - 1)
    a = np.ascontiguousarray(np.broadcast_to(EPS ** (1.0 - t), (n, n)))
    c = np.ascontiguousarray(np.broadcast_to(EPS ** t, (n, n)))
    out = [(a, c)]
    while out[-1][0].shape[0] > 3:
        a, c = out[-1]
        out.append((np.ascontiguousarray(a[0::2, 0::2]), np.ascontiguousarray(c[0::2, 0::2])))
    return out


def right_hand_side(m):
    rng = np.random.default_rng(11)
    b = np.zeros((m + 2,) * 2)
    b[1:-1, 1:-1] = rng.standard_normal((m,) * 2)
    return b


def passes_per_cycle(m, lines, pre=SWEEPS, post=SWEEPS):
    """finest-field passes of one V(pre, post) cycle.  The apply reads u, a, c and writes q: 4.  A point sweep is the apply and
    the smoother's 5; a sweep of two line stages is twice (the apply and the stage's 8).  Between levels: the apply, the
    restriction (reads 2, writes 2 coarse fields) and the prolongation (reads and writes 1, reads 1 coarse field)."""
    sweep = 2 * (4 + 8) if lines else 4 + 5
    sizes = []
    while True:
        sizes.append(float(m * m))
        if m < 3:
            break
        m = (m - 1) // 2
    total = 0.0
    for l, n in enumerate(sizes):
        size = n / sizes[0]
        if l == len(sizes) - 1:
            total += size * sweep * COARSE_SWEEPS
        else:
            r = sizes[l + 1] / n
            total += size * (sweep * (pre + post) + 4 + (2 + 2 * r) + (2 + r))
    return total


# ---------------------------------------------------------------- the same driver in NumPy, on the oracle's operators
def numpy_cycles(texts, interiors, coefs, stages, b, cycles):
    """neptune_hip_mg_solve_lines' cycle as include/neptune_hip.h defines it, one rounding per operation, from x = 0: every
    sweep runs the level's stages (axis, lo, inv, up), each after its own apply -- in order before the coarse correction and
    on the last level, reversed after it; -> x"""
    import neptune_oracle as oracle
    mods = [oracle.Module.parse(t) for t in texts]
    where = [tuple(slice(lo, hi) for lo, hi in zip(*i)) for i in interiors]
    n = len(texts)
    xs = [np.zeros_like(a) for a, _ in coefs]
    rhs = [b.copy()] + [np.zeros_like(a) for a, _ in coefs[1:]]

    def A(l, v):
        out = np.zeros_like(v)
        mods[l].call("entry", out, v, *coefs[l])
        return out

    def stage(l, axis, lo, inv, up):
        w = where[l]
        move = lambda f: np.moveaxis(f[w], axis, 0)
        d = move(rhs[l]) - move(A(l, xs[l]))
        lo, inv, up, x = move(lo), move(inv), move(up), move(xs[l])         # views: x is updated in place
        m = d.shape[0]
        g = [d[0] * inv[0]]
        for i in range(1, m):
            g.append((d[i] - lo[i] * g[i - 1]) * inv[i])
        e = g[m - 1]
        x[m - 1] = x[m - 1] + e
        for i in range(m - 2, -1, -1):
            e = g[i] - up[i] * e
            x[i] = x[i] + e

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

    def cycle(l):
        if l == n - 1:
            for _ in range(COARSE_SWEEPS):
                sweep(l)
            return
        for _ in range(SWEEPS):
            sweep(l)
        t = rhs[l][where[l]] - A(l, xs[l])[where[l]]
        for axis in (1, 0):
            t = weigh(t, axis)
        rhs[l + 1][where[l + 1]] = 4.0 * t
        xs[l + 1][where[l + 1]] = 0.0
        cycle(l + 1)
        e = xs[l + 1][where[l + 1]]
        for axis in (1, 0):
            e = interp(e, axis)
        xs[l][where[l]] = xs[l][where[l]] + e
        for _ in range(SWEEPS):
            sweep(l, reverse=True)

    for _ in range(cycles):
        cycle(0)
    return xs[0]


# ---------------------------------------------------------------- the device
def hierarchy(m, lines):
    """one lowered operator per level; lines: alternating stages (dim 0, then dim 1) from multigrid.line_weights, else point
    Jacobi from multigrid.jacobi_weights; -> (multigrid.Hierarchy, module texts, interiors, coefficient arrays, stage arrays)"""
    from neptune_hip import fields, lowering, multigrid
    F = fields.DeviceField
    levels, texts, interiors, stages = [], [], [], []
    coefs = coefficients(m)
    for l, (a, c) in enumerate(coefs):
        text, interior = build_text(a.shape[0])
        mod = lowering.compile_module(text, dot_entries=(l == 0))
        entry = mod.dot_entry("entry") if l == 0 else mod.geom_entry("entry")
        like = F.from_numpy(np.zeros_like(a))
        others = [F.from_numpy(a), F.from_numpy(c)]
        if lines:
            sts = [multigrid.line_weights(entry, like, interior, axis, others, omega=OMEGA) for axis in (0, 1)]
            levels.append(multigrid.Level(entry, like, interior, others=others, rscale=4.0, lines=sts))
            stages.append([(s.axis, s.lo.numpy(), s.inv.numpy(), s.up.numpy()) for s in sts])
        else:
            minv = multigrid.jacobi_weights(entry, like, interior, others, omega=OMEGA)
            levels.append(multigrid.Level(entry, like, interior, others=others, minv=minv, rscale=4.0))
        texts.append(text)
        interiors.append(interior)
    return multigrid.Hierarchy(levels), texts, interiors, coefs, stages


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 255
    import torch
    from neptune_hip import fields, multigrid
    F = fields.DeviceField

    # 1. Omega = 63^2: the device's x after four cycles with alternating stages against the NumPy driver, bit for bit
    h, texts, interiors, coefs, stages = hierarchy(63, True)
    b = right_hand_side(63)
    x = F.from_numpy(np.zeros_like(b))
    cycles, rr0, rr_last, _ = multigrid.solve(h, x, F.from_numpy(b), pre=SWEEPS, post=SWEEPS, coarse_sweeps=COARSE_SWEEPS, max_cycles=4)
    want = numpy_cycles(texts, interiors, coefs, stages, b, 4)
    got = x.numpy()
    ok = cycles == 4 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    print(f"63^2, {len(h)} levels, alternating line stages, {cycles} cycles: r.r {rr0:.3e} -> {rr_last:.3e}, launches (plain, graph, checks) = "
          f"{multigrid.counts()}, x bit for bit as the NumPy driver on the oracle: {ok}")

    # 2. the size asked for: three solvers to the same r . r
    b = right_hand_side(m)
    bf = F.from_numpy(b)
    hs = {"lines": hierarchy(m, True)[0], "point": hierarchy(m, False)[0]}
    _, rr0, _ = multigrid.cg_solve(hs["point"], F.from_numpy(np.zeros_like(b)), bf, max_iters=0)
    tol2 = RTOL2 * rr0
    results = {}
    for solver, name in (("solve", "lines"), ("solve", "point"), ("cg_solve", "point")):
        for warm in (True, False):                    # the first solve pays first-use tuning and workspace growth
            x = F.from_numpy(np.zeros_like(b))
            work = [F.empty_like(x) for _ in range(3)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if solver == "solve":
                steps, _, rr, _ = multigrid.solve(hs[name], x, bf, pre=SWEEPS, post=SWEEPS, coarse_sweeps=COARSE_SWEEPS,
                                                  max_cycles=MAX_CYCLES, tol2=tol2, check_every=1 if name == "lines" else 4)
            else:
                steps, _, rr = multigrid.cg_solve(hs[name], x, bf, sweeps=SWEEPS, coarse_sweeps=COARSE_SWEEPS, max_iters=MAX_ITERS,
                                                  tol2=tol2, work=work)
            seconds = time.perf_counter() - t0
        results[(solver, name)] = (steps, rr, seconds, x.numpy())
    print(f"{m}^2, eps = {EPS}, the strong direction turning from dim 1 to dim 0 across the domain, V({SWEEPS},{SWEEPS}), omega = {OMEGA}, "
          f"to r.r <= {RTOL2:g} r0.r0 ({len(hs['lines'])} levels):")
    for (solver, name), (steps, rr, seconds, _) in results.items():
        unit = "cycles" if solver == "solve" else "iterations"
        reached = "reached" if rr <= tol2 else f"NOT reached: r.r / r0.r0 = {rr / rr0:.1e}"
        smoother = "alternating line stages" if name == "lines" else "point Jacobi"
        per = f" x {passes_per_cycle(m, name == 'lines'):.1f} passes" if solver == "solve" else ""
        print(f"  multigrid.{solver:<8} {smoother:<24}: {steps} {unit}{per}, {seconds * 1e3:.1f} ms ({reached})")
    ref = results[("cg_solve", "point")][3]
    print(f"  max |u_lines - u_cg| = {float(np.max(np.abs(results[('solve', 'lines')][3] - ref))):.2e}")
    ok = ok and results[("solve", "lines")][1] <= tol2 and results[("cg_solve", "point")][1] <= tol2
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
