#!/usr/bin/env python3
"""A 3-D Poisson problem on a cell-centred grid with MIXED faces, solved by multigrid-preconditioned conjugate gradients on
the symmetric linear transfer pair, beside the constant / averaging pair of DESIGN 3.20.

    A(u)_c = (6 + s_c) u_c - (the six neighbours),   s_c = (+1 per Dirichlet boundary face) + (-1 per Neumann boundary face)

is the 7-point star with the ghost cell mirrored, with its sign flipped on a Dirichlet face (the value 0 on the face) and as it
is on a Neumann one; s is a second input field, so the boundary condition lives in the operator.  Here: the value 0 on the low
face of dimension 0 and on the high face of dimension 2, Neumann faces elsewhere.  One lowered operator per level,
N -> N / 2 -> ... -> 2 (multigrid.coarsening_plan(..., centring="cell")), rscale = 4, damped Jacobi with omega = 0.8.

Level(..., prolong="linear", restrict="linear", faces=...) prolongs with the weights 3/4 and 1/4 and restricts by the
transpose of that, R = P^T / 8, under the same rule per face: the V-cycle is a symmetric preconditioner again, cg_solve takes
it, and a V(1,1) cycle then does about what the constant pair needs V(2,2) for.

Checks: every solve reaches the tolerance; the symmetric pair needs fewer iterations than the constant pair at V(1,1) and no
more at V(2,2); and x of a six-iteration solve on the symmetric pair BIT FOR BIT against the
same driver in NumPy -- one rounding per operation, the operators from the CPU oracle, the scalars of the recurrences taken
from the device's trace (whatever order the device summed in, the fields are then fully determined).

usage: examples/poisson_cell_centred_mgcg.py [N]        (default 64; N = 2^k)"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

RTOL2 = 1e-16
COARSE_SWEEPS = 8
OMEGA = 0.8
MAX_ITERS = 60
FACES = [("dirichlet", "neumann"), ("neumann", "neumann"), ("neumann", "dirichlet")]      # (low, high) per dimension


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
    """s over the (m + 2)^3 box: +1 per Dirichlet and -1 per Neumann boundary face of each interior cell, 0 on the rim"""
    s = np.zeros((m + 2,) * 3)
    for d in range(3):
        for edge, kind in zip((1, m), FACES[d]):
            sl = [slice(1, m + 1)] * 3
            sl[d] = slice(edge, edge + 1)
            s[tuple(sl)] += 1.0 if kind == "dirichlet" else -1.0
    return s


def right_hand_side(n):
    rng = np.random.default_rng(3)
    b = np.zeros((n + 2,) * 3)
    b[(slice(1, -1),) * 3] = rng.standard_normal((n,) * 3)
    return b


# ---------------------------------------------------------------- the same driver in NumPy, on the oracle's operators
def numpy_replay(texts, minvs, ss, b, rz0, trace, sweeps):
    """neptune_hip_mgcg_solve_transfer as include/neptune_hip.h defines it, every pair LINEAR / LINEAR by FACES, one rounding per
    operation, from x = 0, with alpha_k = rz_k / pq_k and beta_k = rz_(k+1) / rz_k taken from the device's rz_0 and trace rows
    (pq_k, rz_(k+1), rr_(k+1)); -> x"""
    import neptune_oracle as oracle
    mods = [oracle.Module.parse(t) for t in texts]
    n = len(texts)
    inner = (slice(1, -1),) * 3
    odd = [(lo == "dirichlet", hi == "dirichlet") for lo, hi in FACES]
    xs = [np.zeros_like(m) for m in minvs]
    rhs = [None] + [np.zeros_like(m) for m in minvs[1:]]

    def A(l, v):
        out = np.zeros_like(v)
        mods[l].call("entry", out, v, ss[l])
        return out

    def sweep(l):
        d = rhs[l][inner] - A(l, xs[l])[inner]
        xs[l][inner] = xs[l][inner] + minvs[l][inner] * d

    def padded(a, axis):
        """a with one ghost on either side along `axis`: + its edge on a Neumann face, - its edge on a Dirichlet one"""
        take = lambda idx: np.take(a, idx, axis=axis)
        first, last = take([0]), take([a.shape[axis] - 1])
        return np.concatenate([-first if odd[axis][0] else first, a, -last if odd[axis][1] else last], axis=axis)

    def gather(a, axis):
        """the transposed restriction along `axis`: 2 m -> m cells"""
        p, j = padded(a, axis), np.arange(a.shape[axis] // 2)
        take = lambda idx: np.take(p, idx, axis=axis)
        u = 0.25 * take(2 * j) + 0.75 * take(2 * j + 1)
        v = 0.75 * take(2 * j + 2) + 0.25 * take(2 * j + 3)
        return 0.5 * (u + v)

    def interpolate(e, axis):
        """the linear prolongation along `axis`: m -> 2 m cells"""
        m = e.shape[axis]
        p = padded(e, axis)
        take = lambda idx: np.take(p, idx, axis=axis)
        own = 0.75 * e
        even = own + 0.25 * take(np.arange(0, m))
        oddc = own + 0.25 * take(np.arange(2, m + 2))
        return np.stack([even, oddc], axis=axis + 1).reshape([2 * v if a == axis else v for a, v in enumerate(e.shape)])

    def cycle(l, first_sweep_done=False):
        if l == n - 1:
            for _ in range(COARSE_SWEEPS):
                sweep(l)
            return
        for _ in range(sweeps - 1 if first_sweep_done else sweeps):
            sweep(l)
        t = rhs[l][inner] - A(l, xs[l])[inner]
        for axis in (2, 1, 0):
            t = gather(t, axis)
        rhs[l + 1][inner] = 4.0 * t
        xs[l + 1][inner] = 0.0
        cycle(l + 1)
        e = xs[l + 1][inner]
        for axis in (2, 1, 0):
            e = interpolate(e, axis)
        xs[l][inner] = xs[l][inner] + e
        for _ in range(sweeps):
            sweep(l)

    def precondition(r):
        """z = M(r): the first pre-sweep of level 0 is z = minv r on the whole box (from z = 0, A(0) = 0)"""
        rhs[0] = r
        xs[0] = minvs[0] * r
        cycle(0, first_sweep_done=True)
        return xs[0].copy()

    x = np.zeros_like(b)
    r = np.zeros_like(b)
    r[inner] = b[inner] - A(0, x)[inner]
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
def hierarchy(n, symmetric):
    """one lowered operator per level of the cell-centred plan; symmetric: every pair linear / linear by FACES, else constant /
    averaging; -> (multigrid.Hierarchy, texts, minv arrays, s arrays)"""
    from neptune_hip import fields, lowering, multigrid
    F = fields.DeviceField
    plan = multigrid.coarsening_plan((n,) * 3, (1.0,) * 3, centring="cell")
    setting = dict(prolong="linear", restrict="linear", faces=FACES) if symmetric else {}
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
    assert h.halved == [p[2] for p in plan[:-1]] and plan[-1][0] == (2, 2, 2) and h.symmetric and h.has_linear_restrict == symmetric
    return h, texts, minvs, ss


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    from neptune_hip import fields, multigrid
    F = fields.DeviceField
    b = right_hand_side(n)
    iters, reached = {}, {}
    for kind in ("constant", "symmetric linear"):
        h, texts, minvs, ss = hierarchy(n, kind != "constant")
        for sweeps in (2, 1):
            x = F.from_numpy(np.zeros_like(b))
            _, rr0, _ = multigrid.cg_solve(h, x, F.from_numpy(b), max_iters=0)
            done, _, rr_last = multigrid.cg_solve(h, x, F.from_numpy(b), sweeps=sweeps, coarse_sweeps=COARSE_SWEEPS, max_iters=MAX_ITERS,
                                                  tol2=RTOL2 * rr0)
            iters[(kind, sweeps)], reached[(kind, sweeps)] = done, rr_last <= RTOL2 * rr0
            print(f"{n}^3 cells, {len(h)} levels down to 2^3, cg_solve around V({sweeps},{sweeps}), {kind} pair: {done} iterations, r.r "
                  f"{rr0:.3e} -> {rr_last:.3e} (reached {RTOL2:g} r0.r0: {reached[(kind, sweeps)]})")
    # the symmetric hierarchy is the last one built: six iterations of V(1,1) against the NumPy driver on the oracle
    x = F.from_numpy(np.zeros_like(b))
    done, _, _, trace = multigrid.cg_solve(h, x, F.from_numpy(b), sweeps=1, coarse_sweeps=COARSE_SWEEPS, max_iters=6, trace=True)
    want = numpy_replay(texts, minvs, ss, b, multigrid.cg_rz0(), trace, sweeps=1)
    same = done == 6 and np.array_equal(x.numpy().view(np.uint64), want.view(np.uint64))
    print(f"x of six iterations on the symmetric linear pair bit for bit as the NumPy driver on the oracle: {same}")
    ok = (same and all(reached.values()) and iters[("symmetric linear", 1)] < iters[("constant", 1)]
          and iters[("symmetric linear", 2)] <= iters[("constant", 2)])
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
