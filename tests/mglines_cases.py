"""The problems of multigrid line smoothers and the factor recurrence of a line stage, exactly as
include/neptune_hip.h defines it -- arithmetic in the element type with one `.astype(dt)` per operation, marched cell by cell
along the line (vectorised across the lines only, which changes no value).  The stage itself, the sweep order and the cycle
are mg_restatement's.

A level is an mg_restatement.Level with `.stages`, a list of (axis, lo, inv, up): empty means the point sweep with minv.

Operators: mg_cases' star for the shape tests (its tridiagonal part along any axis is (-1, 2 rank, -1)), and flux_module,
the symmetric flux form with two cell coefficient fields whose strong direction varies across the domain:
    A(u)_p = 1/2 (a_p + a_(p-e0)) (u_p - u_(p-e0)) + 1/2 (a_p + a_(p+e0)) (u_p - u_(p+e0))
           + 1/2 (c_p + c_(p-e1)) (u_p - u_(p-e1)) + 1/2 (c_p + c_(p+e1)) (u_p - u_(p+e1))
with a = eps^(1 - t), c = eps^t, t = j / (n1 - 1) for physical column j: dim 1 is strong on the left, dim 0 on the right."""
import numpy as np

import mg_cases as mgc
import mg_restatement as rst
import monitor_cases as mc


# ---------------------------------------------------------------- the flux-form operator
def flux_module(shape, dtype=np.float64):
    """NeptuneIR text of @entry(out, u, a, c) on a rank-2 box, bounds one cell in from every face: the operator above, the
    four flux terms added in the order written; all three inputs are read at radius 1"""
    assert len(shape) == 2
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "?x?x" + elem
    acc = [f"        %uc = neptune_ir.access %u0[0, 0] : !temp -> {elem}"]
    ops = [f"        %half = arith.constant 0.5 : {elem}"]
    terms = []
    for d, coef in ((0, "ka"), (1, "kc")):
        acc.append(f"        %{coef}c = neptune_ir.access %{coef}[0, 0] : !temp -> {elem}")
        for sgn, tag in ((-1, "m"), (1, "p")):
            off = [0, 0]
            off[d] = sgn
            n = f"{d}{tag}"
            acc += [f"        %u{n} = neptune_ir.access %u0[{lst(off)}] : !temp -> {elem}",
                    f"        %k{n} = neptune_ir.access %{coef}[{lst(off)}] : !temp -> {elem}"]
            ops += [f"        %s{n} = arith.addf %{coef}c, %k{n} : {elem}", f"        %h{n} = arith.mulf %half, %s{n} : {elem}",
                    f"        %d{n} = arith.subf %uc, %u{n} : {elem}", f"        %t{n} = arith.mulf %h{n}, %d{n} : {elem}"]
            terms.append(f"t{n}")
    ops += [f"        %r0 = arith.addf %{terms[0]}, %{terms[1]} : {elem}", f"        %r1 = arith.addf %r0, %{terms[2]} : {elem}",
            f"        %r2 = arith.addf %r1, %{terms[3]} : {elem}", f"        neptune_ir.yield %r2 : {elem}"]
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [0, 0], ub = [{lst(shape)}]>",
           f"#bi  = #neptune_ir.bounds<lb = [1, 1], ub = [{lst([n - 1 for n in shape])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>, %in1: memref<{mr}>, %in2: memref<{mr}>) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu   = neptune_ir.wrap %in : memref<{mr}> -> !field",
           "    %u    = neptune_ir.load %fu : !field -> !temp",
           f"    %fa   = neptune_ir.wrap %in1 : memref<{mr}> -> !field",
           "    %a    = neptune_ir.load %fa : !field -> !temp",
           f"    %fc   = neptune_ir.wrap %in2 : memref<{mr}> -> !field",
           "    %c    = neptune_ir.load %fc : !field -> !temp",
           "    %r = neptune_ir.apply(%u, %a, %c) attributes {bounds = #bi} : (!temp, !temp, !temp) -> !temp {",
           "      ^bb0(%i0: index, %i1: index, %u0: !temp, %ka: !temp, %kc: !temp):"] + acc + ops + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def flux_coefficients(n, dtype=np.float64, eps=0.01):
    """the cell fields a, c over the n x n box of the finest level: a = eps^(1 - t), c = eps^t, t = j / (n - 1) for column j"""
    t = np.arange(n, dtype=np.float64) / (n - 1)
    a = np.broadcast_to(eps ** (1.0 - t), (n, n)).astype(dtype)
    c = np.broadcast_to(eps ** t, (n, n)).astype(dtype)
    return np.ascontiguousarray(a), np.ascontiguousarray(c)


def flux_tridiagonal(a, c, axis):
    """(lower, diag, upper) of the flux-form operator along `axis` on Omega = one cell in from every face, +0 elsewhere and
    for couplings to the rim, from a and c alone, in their element type with the module's order of operations"""
    dt = a.dtype.type
    k = (a, c)
    inner = (slice(1, -1), slice(1, -1))

    def half_sum(f, d, sgn):
        sh = [slice(1, -1), slice(1, -1)]
        sh[d] = slice(1 + sgn, f.shape[d] - 1 + sgn)
        return (dt(0.5) * (f[inner] + f[tuple(sh)]).astype(dt)).astype(dt)
    h = [half_sum(k[d], d, sgn) for d in (0, 1) for sgn in (-1, 1)]       # 0m, 0p, 1m, 1p
    diag = (((h[0] + h[1]).astype(dt) + h[2]).astype(dt) + h[3]).astype(dt)
    lower, upper = -h[2 * axis], -h[2 * axis + 1]
    first, last = [slice(None)] * 2, [slice(None)] * 2
    first[axis], last[axis] = 0, -1
    lower[tuple(first)] = dt(0)
    upper[tuple(last)] = dt(0)
    out = []
    for f in (lower, diag, upper):
        full = np.zeros(a.shape, a.dtype)
        full[inner] = f
        out.append(full)
    return tuple(out)


# ---------------------------------------------------------------- the factor recurrence
def factors(lower, diag, upper, where, axis, omega, outside=0.0):
    """Thomas's elimination of T / omega along `axis` on Omega: -> (lo, inv, up) over the box; `outside` (+0 by definition;
    NaN proves it is never read) on every cell outside Omega, +0 for lo at i = 0 and up at i = m - 1.  ValueError on a
    pivot that is 0 or not finite."""
    dt = diag.dtype.type
    w = dt(omega)
    view = lambda f: np.moveaxis(f[where], axis, 0)
    l, t, u = view(lower), view(diag), view(upper)
    m = t.shape[0]
    lo, inv, up = (np.zeros(t.shape, diag.dtype) for _ in range(3))
    c_prev = None
    with np.errstate(all="ignore"):
        for i in range(m):
            li, ti, ui = (l[i] / w).astype(dt), (t[i] / w).astype(dt), (u[i] / w).astype(dt)
            if i == 0:
                den = ti
            else:
                p = (li * c_prev).astype(dt)
                den = (ti - p).astype(dt)
                lo[i] = li
            if ((den == 0) | ~np.isfinite(den)).any():
                raise ValueError(f"a pivot at interior index {i} is 0 or not finite")
            inv[i] = (dt(1) / den).astype(dt)
            c_prev = (ui * inv[i]).astype(dt)
            if i < m - 1:
                up[i] = c_prev
    out = []
    for f in (lo, inv, up):
        full = np.full(diag.shape, outside, diag.dtype)
        full[where] = np.moveaxis(f, 0, axis)
        out.append(full)
    return tuple(out)


# ---------------------------------------------------------------- hierarchies
def star_tridiagonal(shape, where, dtype):
    """the tridiagonal part of mg_cases' star along any axis except for the rim couplings: (-1, 2 rank, -1) on Omega"""
    lower, diag, upper = (np.zeros(shape, dtype) for _ in range(3))
    lower[where], diag[where], upper[where] = -1.0, 2.0 * len(shape), -1.0
    return lower, diag, upper


def star_stage(L, axis, damp, outside=np.nan):
    """a stage of the star operator on restatement level L along `axis` (rim couplings dropped)"""
    lower, diag, upper = star_tridiagonal(L.shape, L.where, L.dt)
    first, last = list(L.where), list(L.where)
    first[axis] = L.where[axis].start
    last[axis] = L.where[axis].stop - 1
    lower[tuple(first)] = 0.0
    upper[tuple(last)] = 0.0
    return (axis,) + factors(lower, diag, upper, L.where, axis, damp, outside)


def star_levels(omega, n_levels, dtype, damp, stage_axes, texts=None):
    """mg_cases.star_levels with line stages: stage_axes[l] = the axes of level l's stages, in order (() = point Jacobi)"""
    levels, texts = mgc.star_levels(omega, n_levels, dtype, damp, texts)
    for L, axes in zip(levels, stage_axes):
        L.stages = [star_stage(L, a, damp) for a in axes]
    return levels, texts


FLUX_N, FLUX_DAMP, FLUX_EPS = 65, 0.8, 0.01


def flux_levels(stage_axes=(0, 1), n=FLUX_N, damp=FLUX_DAMP, dtype=np.float64, eps=FLUX_EPS, outside=np.nan):
    """the hierarchy of the varying-anisotropy problem: boxes n, (n + 1) / 2, ... down to 3 (Omega n - 2 -> ... -> 1), the
    coefficients injected (a[0::2, 0::2] on the box), rscale = 4; every level carries minv = damp / diagonal and one stage
    per axis in stage_axes (() = point Jacobi); -> (levels, texts, [(a_l, c_l)])"""
    dt = np.dtype(dtype).type
    a, c = flux_coefficients(n, dtype, eps)
    levels, texts, coefs = [], [], []
    while True:
        shape = a.shape
        where = (slice(1, shape[0] - 1), slice(1, shape[1] - 1))
        text = flux_module(shape, dtype)
        minv = np.full(shape, outside, dtype)
        minv[where] = (dt(damp) / flux_tridiagonal(a, c, 0)[1][where]).astype(dt)
        L = rst.Level(rst.Operator(text, a, c), shape, where, minv, dtype)
        L.stages = [(ax,) + factors(*flux_tridiagonal(a, c, ax), where, ax, damp, outside) for ax in stage_axes]
        levels.append(L)
        texts.append(text)
        coefs.append((a, c))
        if shape[0] <= 3:
            return levels, texts, coefs
        a, c = np.ascontiguousarray(a[0::2, 0::2]), np.ascontiguousarray(c[0::2, 0::2])


def flux_problem(levels, seed=2024):
    """x0 = 0 and b standard normal (a fixed seed), in level 0's element type"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(levels[0].shape).astype(levels[0].dt)
    return np.zeros(levels[0].shape, levels[0].dt), b


def stage_applications(levels, sweeps, coarse_sweeps):
    """how many line stages (or point sweeps) one cycle applies over all levels"""
    total = 0
    for l, L in enumerate(levels):
        k = max(len(getattr(L, "stages", [])), 1)
        total += k * (coarse_sweeps if l == len(levels) - 1 else 2 * sweeps)
    return total
