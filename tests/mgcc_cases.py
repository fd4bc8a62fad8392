"""The problems of multigrid on cell-centred grids.

Between two neighbouring levels a dimension may be HALVED, m_fine = 2 m_coarse: the coarse cell j covers the fine cells 2 j
and 2 j + 1.  A level carries `.axes` as everywhere else; for a cell-centred pair it is a Halved(...) -- a plain tuple is a
vertex-centred pair, so a hierarchy may change its grid kind from one pair to the next.  The transfers, the cycle, the solve
and MGCG are mg_restatement's.

Operators: flux_module, the flux form with one face-coefficient field per dimension and an optional diagonal field,
    A(u)_p = sum_d [ c_d[p] (u_p - u_(p - e_d)) + c_d[p + e_d] (u_p - u_(p + e_d)) ]  (+ s[p] u_p),
c_d[p] the coefficient of the face between cells p - e_d and p.  Neumann faces: c = 0 on the boundary faces.  Dirichlet
faces (the value 0 on the face itself, the ghost cell mirrored): c = 0 there as well and s = 2 per boundary face of the cell.
The operator is unscaled (h^2 A) with rscale = 4: a level's interior coefficients along dimension d are a weight w_d that
follows the plan rule of mgsemi_cases (w on a halved dimension, 4 w on a kept one), 1 everywhere under full halving."""
import numpy as np

import mg_restatement as rst
import monitor_cases as mc
from mg_restatement import Halved


# ---------------------------------------------------------------- the flux-form operator
def flux_module(shape, dtype=np.float64, diagonal=False):
    """NeptuneIR text of @entry(out, u, c_0 .. c_(rank-1)[, s]), bounds one cell in from every face: the operator of the module
    docstring, the terms added in the order written (per dimension the lower face, then the upper one; s u_p last); every
    input has u's box, c_d is read at p and p + e_d"""
    rank = len(shape)
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "x".join(["?"] * rank) + "x" + elem
    zero = [0] * rank
    n_in = rank + (2 if diagonal else 1)
    body = [f"        %uc = neptune_ir.access %u0[{lst(zero)}] : !temp -> {elem}"]
    terms = []
    for d in range(rank):
        lo, hi = list(zero), list(zero)
        lo[d], hi[d] = -1, 1
        body += [f"        %um{d} = neptune_ir.access %u0[{lst(lo)}] : !temp -> {elem}",
                 f"        %up{d} = neptune_ir.access %u0[{lst(hi)}] : !temp -> {elem}",
                 f"        %km{d} = neptune_ir.access %k{d}[{lst(zero)}] : !temp -> {elem}",
                 f"        %kp{d} = neptune_ir.access %k{d}[{lst(hi)}] : !temp -> {elem}",
                 f"        %dm{d} = arith.subf %uc, %um{d} : {elem}", f"        %tm{d} = arith.mulf %km{d}, %dm{d} : {elem}",
                 f"        %dp{d} = arith.subf %uc, %up{d} : {elem}", f"        %tp{d} = arith.mulf %kp{d}, %dp{d} : {elem}"]
        terms += [f"tm{d}", f"tp{d}"]
    if diagonal:
        body += [f"        %sg = neptune_ir.access %ks[{lst(zero)}] : !temp -> {elem}", f"        %ts = arith.mulf %sg, %uc : {elem}"]
        terms.append("ts")
    body.append(f"        %r1 = arith.addf %{terms[0]}, %{terms[1]} : {elem}")
    for i, t in enumerate(terms[2:], start=2):
        body.append(f"        %r{i} = arith.addf %r{i - 1}, %{t} : {elem}")
    body.append(f"        neptune_ir.yield %r{len(terms) - 1} : {elem}")
    names = ["u"] + [f"c{d}" for d in range(rank)] + (["s"] if diagonal else [])
    args = ", ".join(f"%in{i if i else ''}: memref<{mr}>" for i in range(n_in))
    loads = []
    for i, nm in enumerate(names):
        loads += [f"    %f{nm} = neptune_ir.wrap %in{i if i else ''} : memref<{mr}> -> !field",
                  f"    %{nm} = neptune_ir.load %f{nm} : !field -> !temp"]
    block = ", ".join([f"%i{d}: index" for d in range(rank)] + ["%u0: !temp"] + [f"%k{d}: !temp" for d in range(rank)] +
                      (["%ks: !temp"] if diagonal else []))
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(zero)}], ub = [{lst(shape)}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst([1] * rank)}], ub = [{lst([n - 1 for n in shape])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, {args}) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field"] + loads + [
           f"    %r = neptune_ir.apply({', '.join('%' + nm for nm in names)}) attributes {{bounds = #bi}} : "
           f"({', '.join(['!temp'] * n_in)}) -> !temp {{",
           f"      ^bb0({block}):"] + body + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def face_fields(m, dtype, faces, weights=None):
    """the operator's fixed inputs over the box of a level with interior extents `m` (rim of one cell) and its diagonal:
    -> ([c_0 .. c_(rank-1)] (+ [s] for faces = "dirichlet"), diag), c_d = weights[d] (default 1) on the interior faces and 0
    on the boundary faces and everywhere else, s = 2 weights[d] per boundary face; diag = the sum of the cell's face coefficients (+ s), in the element type and the module's
    order, on Omega and +0 elsewhere"""
    assert faces in ("neumann", "dirichlet")
    rank = len(m)
    dt = np.dtype(dtype).type
    w = [1.0] * rank if weights is None else [float(v) for v in weights]
    shape = tuple(n + 2 for n in m)
    where = tuple(slice(1, 1 + n) for n in m)
    cs = []
    for d in range(rank):
        c = np.zeros(shape, dtype)
        sl = list(where)
        sl[d] = slice(2, 1 + m[d])          # the faces between two cells of Omega
        c[tuple(sl)] = w[d]
        cs.append(c)
    rest = list(cs)
    if faces == "dirichlet":
        s = np.zeros(shape, dtype)
        for d in range(rank):
            for edge in (1, m[d]):
                sl = list(where)
                sl[d] = slice(edge, edge + 1)
                s[tuple(sl)] += dt(2 * w[d])
        rest.append(s)
    diag = np.zeros(shape, dtype)
    acc = None
    for d in range(rank):
        up = list(where)
        up[d] = slice(2, 2 + m[d])
        for t in (cs[d][where], cs[d][tuple(up)]):
            acc = t.copy() if acc is None else (acc + t).astype(dt)
    if faces == "dirichlet":
        acc = (acc + rest[-1][where]).astype(dt)
    diag[where] = acc
    return rest, diag


def halved_steps(omega, axes_per_pair, weights=None):
    """[(extents, weights, axes)] for a hierarchy given per pair by a Halved(...) (m / 2 along them) or a plain tuple
    (vertex-centred: (m - 1) / 2 along them), the weights by the plan rule (w on such a dimension, 4 w on a kept one);
    axes = () on the last level"""
    m, out = tuple(int(v) for v in omega), []
    w = tuple(1.0 for _ in m) if weights is None else tuple(float(v) for v in weights)
    for axes in axes_per_pair:
        out.append((m, w, axes))
        w = tuple(v if d in axes else 4.0 * v for d, v in enumerate(w))
        if rst.pair_of(axes, len(m)).halved:
            assert all(m[d] % 2 == 0 and m[d] >= 2 for d in axes), (m, axes)
            m = tuple(v // 2 if d in axes else v for d, v in enumerate(m))
        else:
            assert all(m[d] % 2 == 1 and m[d] >= 3 for d in axes), (m, axes)
            m = tuple((v - 1) // 2 if d in axes else v for d, v in enumerate(m))
    out.append((m, w, ()))
    return out


def plan(extents, weights=None, threshold=0.5, max_levels=16):
    """the rule of multigrid.coarsening_plan(..., centring="cell"), restated: a dimension can be halved when its extent is
    even and >= 4; of those, the ones whose weight is at least threshold x the largest among them are; -> [(extents, weights,
    axes)], axes a Halved(...), () on the last level.  Every extent ends at 2 or at an odd number."""
    m = tuple(int(v) for v in extents)
    w = tuple(1.0 for _ in m) if weights is None else tuple(float(v) for v in weights)
    out = []
    while True:
        can = [d for d, v in enumerate(m) if v % 2 == 0 and v >= 4]
        if not can or len(out) + 1 >= max_levels:
            out.append((m, w, ()))
            return out
        top = max(w[d] for d in can)
        axes = Halved(d for d in can if w[d] >= threshold * top)
        out.append((m, w, axes))
        m = tuple(v // 2 if d in axes else v for d, v in enumerate(m))
        w = tuple(v if d in axes else 4.0 * v for d, v in enumerate(w))


def flux_levels(steps, damp, dtype=np.float64, faces="neumann", outside0=0.0):
    """restatement levels (whole-interior boxes, rim of one cell), module texts and the fixed inputs per level for
    [(extents, weights, axes)]: minv = damp / diag on Omega (one division in the element type); outside Omega level 0's minv is
    `outside0` (MGCG forms minv_0 * r on the whole box), the coarser levels' NaN (never read); -> (levels, texts, rests)"""
    dt = np.dtype(dtype).type
    levels, texts, rests = [], [], []
    for l, (m, w, axes) in enumerate(steps):
        shape = tuple(n + 2 for n in m)
        where = tuple(slice(1, 1 + n) for n in m)
        text = flux_module(shape, dtype, diagonal=faces == "dirichlet")
        rest, diag = face_fields(m, dtype, faces, w)
        minv = np.full(shape, outside0 if l == 0 else np.nan, dtype)
        with np.errstate(divide="ignore"):
            minv[where] = (dt(damp) / diag[where]).astype(dt)
        L = rst.Level(rst.Operator(text, *rest), shape, where, minv, dtype)
        L.axes, L.weights = axes, w
        levels.append(L)
        texts.append(text)
        rests.append(rest)
    return levels, texts, rests


def compatible(b, where):
    """b with its mean over Omega taken off on Omega (formed in float64, rounded once): a right-hand side the pure-Neumann
    operator can serve"""
    out = b.copy()
    out[where] = (b[where].astype(np.float64) - np.mean(b[where], dtype=np.float64)).astype(b.dtype)
    return out


def dense(fn, n_in, n_out):
    """the matrix of a linear map on flat float64 vectors, column by column"""
    M = np.zeros((n_out, n_in))
    for j in range(n_in):
        e = np.zeros(n_in)
        e[j] = 1.0
        M[:, j] = fn(e)
    return M
