#!/usr/bin/env python3
"""A 3-D Poisson problem on a cell-centred grid, the value 0 ON every face, solved by PLAIN multigrid cycles: piecewise-constant
against linear prolongation, beside multigrid.cg_solve.

    A(u)_c = (6 + s_c) u_c - (the six neighbours),   s_c = the number of boundary faces of the cell c

is the 7-point star with the ghost cell mirrored with its sign flipped (u_ghost = -u_c puts the value 0 on the face); s is a
second input field, so the boundary condition lives in the operator.  One lowered operator per level, N -> N / 2 -> ... -> 2
(multigrid.coarsening_plan(..., centring="cell")), rscale = 4, damped Jacobi with omega = 0.8.

With the constant prolongation plain cycles are not grid-independent (at large N they stall or diverge, which is why
cg_solve is wrapped around them); with Level(..., prolong="linear", faces="dirichlet") -- weights 3/4 and 1/4, the ghost of a
coarse edge cell its negative -- they converge at a rate that does not move with N.  The linear pair is not a symmetric
preconditioner, so cg_solve refuses it and runs on the constant hierarchy here.

Checks: linear needs fewer cycles than constant and reaches the tolerance; cg_solve refuses the linear hierarchy; and the
linear solve's x BIT FOR BIT against the same driver in NumPy -- one rounding per operation, the operators from the CPU
oracle (no reduction enters a field).

usage: examples/poisson_cell_centred_multigrid.py [N]        (default 64; N = 2^k)"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

RTOL2 = 1e-16
SWEEPS, COARSE_SWEEPS = 2, 8
OMEGA = 0.8
MAX_CYCLES = 40


def operator_text(m):
    """@entry(out, u, s): out = (6 + s) u - (the six neighbours) on the interior m^3 of a box two cells larger per dimension"""
    import neptune as nep
    nep.reset()
    box = ([0, 0, 0], [m + 2] * 3)
    interior = ([1, 1, 1], [m + 1] * 3)
    c = nep.get_compiler()
    c.start_function("entry", [("memref", 3)] * 3)
    fout = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    u, s = (nep.load(nep.wrap(nep.Expr(c.get_function_arg(1 + i)), box)) for i in range(2))

    @nep.apply(inputs=[u, s], bounds=interior)
    def star(x, d):
        return (x[0, 0, 0] * 6.0 - ((x[-1, 0, 0] + x[1, 0, 0]) + (x[0, -1, 0] + x[0, 1, 0]) + (x[0, 0, -1] + x[0, 0, 1]))) + d[0, 0, 0] * x[0, 0, 0]

    nep.store(star, fout)
    c.create_return(nep.unwrap(fout)._handle)
    c.end_function()
    text = c.dump()
    nep.reset()
    return text, interior


def boundary_faces(m):
    """s over the (m + 2)^3 box: the number of boundary faces of each interior cell, 0 on the rim"""
    s = np.zeros((m + 2,) * 3)
    for d in range(3):
        for edge in (1, m):
            sl = [slice(1, m + 1)] * 3
            sl[d] = slice(edge, edge + 1)
            s[tuple(sl)] += 1.0
    return s


def right_hand_side(n):
    rng = np.random.default_rng(3)
    b = np.zeros((n + 2,) * 3)
    b[(slice(1, -1),) * 3] = rng.standard_normal((n,) * 3)
    return b


# ---------------------------------------------------------------- the same driver in NumPy, on the oracle's operators
def numpy_cycles(texts, minvs, ss, b, cycles, linear):
    """`cycles` cycles of neptune_hip_mg_solve_prolong as include/neptune_hip.h defines it, from x = 0, every pair halving every
    dimension, one rounding per operation; linear: every pair LINEAR with rule ODD on every face; -> x"""
    import neptune_oracle as oracle
    mods = [oracle.Module.parse(t) for t in texts]
    n = len(texts)
    inner = (slice(1, -1),) * 3
    xs = [np.zeros_like(m) for m in minvs]
    rhs = [np.zeros_like(m) for m in minvs]
    rhs[0] = b.copy()

    def A(l, v):
        out = np.zeros_like(v)
        mods[l].call("entry", out, v, ss[l])
        return out

    def sweep(l):
        d = rhs[l][inner] - A(l, xs[l])[inner]
        xs[l][inner] = xs[l][inner] + minvs[l][inner] * d

    def mean(t, axis):
        k = t.shape[axis]
        return 0.5 * (np.take(t, np.arange(0, k, 2), axis=axis) + np.take(t, np.arange(1, k, 2), axis=axis))

    def interpolate(e, axis):
        m = e.shape[axis]
        take = lambda a, idx: np.take(a, idx, axis=axis)
        padded = np.concatenate([-take(e, [0]), e, -take(e, [m - 1])], axis=axis)     # rule ODD: the ghost is minus the edge
        p = 0.75 * e
        even = p + 0.25 * take(padded, np.arange(0, m))
        odd = p + 0.25 * take(padded, np.arange(2, m + 2))
        return np.stack([even, odd], axis=axis + 1).reshape([2 * v if a == axis else v for a, v in enumerate(e.shape)])

    def cycle(l):
        if l == n - 1:
            for _ in range(COARSE_SWEEPS):
                sweep(l)
            return
        for _ in range(SWEEPS):
            sweep(l)
        t = rhs[l][inner] - A(l, xs[l])[inner]
        for axis in (2, 1, 0):
            t = mean(t, axis)
        rhs[l + 1][inner] = 4.0 * t
        xs[l + 1][inner] = 0.0
        cycle(l + 1)
        e = xs[l + 1][inner]
        for axis in (2, 1, 0):
            e = interpolate(e, axis) if linear else np.repeat(e, 2, axis=axis)
        xs[l][inner] = xs[l][inner] + e
        for _ in range(SWEEPS):
            sweep(l)

    for _ in range(cycles):
        cycle(0)
    return xs[0]


# ---------------------------------------------------------------- the device
def hierarchy(n, linear):
    """one lowered operator per level of the cell-centred plan; -> (multigrid.Hierarchy, texts, minv arrays, s arrays)"""
    from neptune_hip import fields, lowering, multigrid
    F = fields.DeviceField
    plan = multigrid.coarsening_plan((n,) * 3, (1.0,) * 3, centring="cell")
    setting = dict(prolong="linear", faces="dirichlet") if linear else {}
    levels, texts, minvs, ss = [], [], [], []
    for l, (extents, _, _) in enumerate(plan):
        m = extents[0]
        text, interior = operator_text(m)
        mod = lowering.compile_module(text, dot_entries=(l == 0))
        entry = mod.dot_entry("entry") if l == 0 else mod.geom_entry("entry")
        like = F.from_numpy(np.zeros((m + 2,) * 3))
        s = boundary_faces(m)
        others = [F.from_numpy(s)]
        minv = multigrid.jacobi_weights(entry, like, interior, others=others, omega=OMEGA, reach=1)
        levels.append(multigrid.Level(entry, like, interior, others=others, minv=minv, rscale=4.0, **setting))
        texts.append(text)
        minvs.append(minv.numpy())
        ss.append(s)
    h = multigrid.Hierarchy(levels)
    assert h.halved == [p[2] for p in plan[:-1]] and plan[-1][0] == (2, 2, 2) and h.has_linear == linear
    return h, texts, minvs, ss


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    from neptune_hip import fields, multigrid
    F = fields.DeviceField
    b = right_hand_side(n)
    schedule = dict(pre=SWEEPS, post=SWEEPS, coarse_sweeps=COARSE_SWEEPS)
    done = {}
    for kind in ("constant", "linear"):
        h, texts, minvs, ss = hierarchy(n, kind == "linear")
        x = F.from_numpy(np.zeros_like(b))
        _, rr0, _, _ = multigrid.solve(h, x, F.from_numpy(b), max_cycles=0)
        cycles, _, rr_last, checks = multigrid.solve(h, x, F.from_numpy(b), max_cycles=MAX_CYCLES, tol2=RTOL2 * rr0, **schedule)
        factors = [a / c for a, c in zip([rr0] + checks, checks)]
        done[kind] = (cycles, rr_last <= RTOL2 * rr0)
        print(f"{n}^3 cells, {len(h)} levels down to 2^3, V({SWEEPS},{SWEEPS}) plain cycles, {kind} prolongation: {cycles} cycles, r.r "
              f"{rr0:.3e} -> {rr_last:.3e} (reached {RTOL2:g} r0.r0: {done[kind][1]}); r.r factor per cycle, last three: "
              + ", ".join(f"{f:.1f}" for f in factors[-3:]))
        if kind == "constant":
            xg = F.from_numpy(np.zeros_like(b))
            iters, _, rr_cg = multigrid.cg_solve(h, xg, F.from_numpy(b), sweeps=SWEEPS, coarse_sweeps=COARSE_SWEEPS, max_iters=MAX_CYCLES,
                                                 tol2=RTOL2 * rr0)
            print(f"  cg_solve around the same cycle: {iters} iterations, r.r -> {rr_cg:.3e}")
            cg_ok = rr_cg <= RTOL2 * rr0
    try:
        multigrid.cg_solve(h, x, F.from_numpy(b))
        refused = False
    except ValueError as err:
        refused = "symmetric" in str(err)
    want = numpy_cycles(texts, minvs, ss, b, done["linear"][0], linear=True)
    same = np.array_equal(x.numpy().view(np.uint64), want.view(np.uint64))
    print(f"cg_solve refuses the linear hierarchy: {refused}; x of the linear solve bit for bit as the NumPy driver on the oracle: {same}")
    ok = same and refused and cg_ok and done["linear"][1] and done["linear"][0] < done["constant"][0]
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
