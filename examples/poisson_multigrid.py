#!/usr/bin/env python3
"""3-D Poisson by geometric multigrid on the device:

    6 u - (six neighbours of u) = b      on the interior Omega = M^3, u = 0 on the rim

The operator's diagonal is constant, so a Jacobi preconditioner does nothing for conjugate gradients and their iteration
count grows with M.  A V-cycle does not care: neptune_hip.multigrid.solve (neptune_hip_mg_solve) smooths with
damped Jacobi, restricts the residual by full weighting, corrects by trilinear interpolation, and brings r . r down by more
than an order of magnitude per cycle whatever M is.  Every level's operator is the same stencil lowered from the Python DSL
for that level's shape (one module per level; rscale = 4 because the stencil carries no 1 / h^2).

The script solves to r . r <= 1e-16 r0 . r0 with multigrid.solve and with apply.cg_solve, and prints cycles against
iterations and the field passes both paid (a pass = one read or write of a finest-level field; counts, not timings).  First,
at Omega = 31^3 (five levels), the multigrid solution is checked BIT FOR BIT against the same driver in NumPy -- one rounding
per operation, the operator from the CPU oracle: no reduction enters a field, so the fields of a run are fully determined.

usage: examples/poisson_multigrid.py [M]        (default 255: Omega = 255^3, eight levels; M = 2^k - 1)"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

RTOL2 = 1e-16
PRE, POST, COARSE_SWEEPS = 2, 2, 8
OMEGA = 6.0 / 7.0      # the damping that makes Jacobi the best smoother for the 7-point star
MAX_CYCLES, MAX_ITERS, CHECK_EVERY_CG = 40, 4000, 10


def build_text(m):
    """@entry(out, u): out = 6 u - (six neighbours) on the interior m^3 of a box (m + 2)^3, copy-through on the rim"""
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
    def poisson(x):
        return x[0, 0, 0] * 6.0 - (x[-1, 0, 0] + x[1, 0, 0] + x[0, -1, 0] + x[0, 1, 0] + x[0, 0, -1] + x[0, 0, 1])

    nep.store(poisson, fout)
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
    x = (np.arange(m + 2)) / (m + 1)
    s = np.sin(np.pi * x) + 0.25 * np.sin(7 * np.pi * x)
    b = s[:, None, None] * s[None, :, None] * s[None, None, :]
    rng = np.random.default_rng(11)
    return b + 0.5 * rng.standard_normal(b.shape)          # rough as well as smooth: every level has work to do


def passes_per_cycle(n_levels, rank=3):
    """finest-field passes of one V(PRE, POST) cycle: 7 per sweep (apply 2, smoother 5), apply + restriction, prolongation"""
    total = 0.0
    for l in range(n_levels):
        size = 1.0 / (2 ** rank) ** l
        if l == n_levels - 1:
            total += size * 7 * COARSE_SWEEPS
        else:
            total += size * (7 * (PRE + POST) + 2 + (2 + 2 / 2 ** rank) + (2 + 1 / 2 ** rank))
    return total


# ---------------------------------------------------------------- the same driver in NumPy, on the oracle's operator
def numpy_solve(texts, interiors, minvs, b, cycles):
    """`cycles` V-cycles as include/neptune_hip.h defines them, one rounding per operation; -> x of level 0"""
    import neptune_oracle as oracle
    mods = [oracle.Module.parse(t) for t in texts]
    where = [tuple(slice(lo, hi) for lo, hi in zip(*i)) for i in interiors]
    n = len(texts)
    x = [np.zeros_like(m) for m in minvs]
    rhs = [b.copy()] + [np.zeros_like(m) for m in minvs[1:]]

    def A(l, v):
        out = np.zeros_like(v)
        mods[l].call("entry", out, v)
        return out

    def sweep(l):
        w = where[l]
        d = rhs[l][w] - A(l, x[l])[w]
        x[l][w] = x[l][w] + minvs[l][w] * d

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
        for _ in range(PRE):
            sweep(l)
        t = rhs[l][where[l]] - A(l, x[l])[where[l]]
        for axis in (2, 1, 0):
            t = weigh(t, axis)
        rhs[l + 1][where[l + 1]] = 4.0 * t
        x[l + 1][where[l + 1]] = 0.0
        cycle(l + 1)
        e = x[l + 1][where[l + 1]]
        for axis in (2, 1, 0):
            e = interp(e, axis)
        x[l][where[l]] = x[l][where[l]] + e
        for _ in range(POST):
            sweep(l)

    for _ in range(cycles):
        cycle(0)
    return x[0]


# ---------------------------------------------------------------- the device
def hierarchy(m):
    """-> (multigrid.Hierarchy, level-0 entry with its dot entry, level-0 interior, module texts, interiors, minv arrays)"""
    from neptune_hip import fields, lowering, multigrid
    F = fields.DeviceField
    levels, texts, interiors, minvs = [], [], [], []
    entry0 = None
    for l, ml in enumerate(level_extents(m)):
        text, interior = build_text(ml)
        mod = lowering.compile_module(text, dot_entries=(l == 0))
        entry = mod.dot_entry("entry") if l == 0 else mod.geom_entry("entry")
        entry0 = entry0 or entry
        like = F.from_numpy(np.zeros((ml + 2,) * 3))
        minv = multigrid.jacobi_weights(entry, like, interior, omega=OMEGA)
        levels.append(multigrid.Level(entry, like, interior, minv=minv, rscale=4.0))
        texts.append(text)
        interiors.append(interior)
        minvs.append(minv.numpy())
    return multigrid.Hierarchy(levels), entry0, interiors[0], texts, interiors, minvs


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 255
    import torch
    from neptune_hip import apply, fields, multigrid
    F = fields.DeviceField

    # 1. Omega = 31^3, five levels: the device's x against the NumPy driver on the oracle, bit for bit
    h, _, _, texts, interiors, minvs = hierarchy(31)
    b = right_hand_side(31)
    x = F.from_numpy(np.zeros_like(b))
    cycles, rr0, rr_last, _ = multigrid.solve(h, x, F.from_numpy(b), pre=PRE, post=POST, coarse_sweeps=COARSE_SWEEPS, max_cycles=4)
    want = numpy_solve(texts, interiors, minvs, b, cycles)
    got = x.numpy()
    ok = len(h) == 5 and cycles == 4 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    print(f"31^3, {len(h)} levels, {cycles} cycles: r.r {rr0:.3e} -> {rr_last:.3e}, launches (plain, graph, checks) = "
          f"{multigrid.counts()}, x bit for bit as the NumPy driver on the oracle: {ok}")

    # 2. the size asked for: multigrid against conjugate gradients, to the same r . r
    h, entry, interior, _, _, _ = hierarchy(m)
    b = right_hand_side(m)
    bf = F.from_numpy(b)
    per_cycle = passes_per_cycle(len(h))
    for warm in (True, False):                    # the first solve pays first-use tuning and workspace growth
        x = F.from_numpy(np.zeros_like(b))
        _, rr0, _, _ = multigrid.solve(h, x, bf, max_cycles=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cycles, _, rr_mg, _ = multigrid.solve(h, x, bf, pre=PRE, post=POST, coarse_sweeps=COARSE_SWEEPS, max_cycles=MAX_CYCLES,
                                              tol2=RTOL2 * rr0)
        t_mg = time.perf_counter() - t0
        xc = F.from_numpy(np.zeros_like(b))
        work = [F.empty_like(xc) for _ in range(3)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iters, _, rr_cg = apply.cg_solve(entry, xc, bf, interior, MAX_ITERS, RTOL2 * rr0, check_every=CHECK_EVERY_CG, work=work)
        t_cg = time.perf_counter() - t0
    ok = ok and rr_mg <= RTOL2 * rr0 and rr_cg <= RTOL2 * rr0
    diff = float(np.max(np.abs(x.numpy() - xc.numpy())))
    print(f"{m}^3, {len(h)} levels, to r.r <= {RTOL2:g} r0.r0:")
    print(f"  multigrid V({PRE},{POST}): {cycles} cycles x {per_cycle:.1f} passes = {cycles * per_cycle:.0f} passes "
          f"(+ 4 per check), {t_mg * 1e3:.1f} ms")
    print(f"  conjugate gradients: {iters} iterations x 11 passes = {iters * 11} passes, {t_cg * 1e3:.1f} ms")
    print(f"  max |u_mg - u_cg| = {diff:.2e}")
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
