"""The problems of the linear prolongation on cell-centred pairs: a pair that prolongs linearly carries a
Linear(axes, rim), .rim[d] = (low rule, high rule) per field dimension, EVEN for a Neumann face and ODD for a Dirichlet one;
operators whose two faces of a dimension may differ.  The transfers and the cycle are mg_restatement's."""
import numpy as np

import mg_cases as mgc
import mg_restatement as rst
import mgcc_cases as cc
from mg_restatement import Linear


# ---------------------------------------------------------------- hierarchies
def linear_steps(steps, rim, only=None):
    """mgcc_cases' steps [(extents, weights, axes)] with every Halved pair (or the pairs listed in `only`) made Linear"""
    out = []
    for l, (m, w, axes) in enumerate(steps):
        if rst.pair_of(axes, len(m)).halved and len(axes) and (only is None or l in only):
            axes = Linear(axes, rim)
        out.append((m, w, axes))
    return out


def mixed_face_fields(m, dtype, faces, weights=None):
    """mgcc_cases.face_fields for a (low, high) pair of "neumann" / "dirichlet" per dimension: -> ([c_0 .. c_(rank-1), s],
    diag); s = 2 weights[d] per Dirichlet boundary face of the cell (0 on a Neumann one), the diagonal field always present"""
    rank = len(m)
    dt = np.dtype(dtype).type
    w = [1.0] * rank if weights is None else [float(v) for v in weights]
    rest, _ = cc.face_fields(m, dtype, "dirichlet", w)
    shape = tuple(n + 2 for n in m)
    where = tuple(slice(1, 1 + n) for n in m)
    s = np.zeros(shape, dtype)
    for d in range(rank):
        for edge, kind in zip((1, m[d]), faces[d]):
            if kind == "dirichlet":
                sl = list(where)
                sl[d] = slice(edge, edge + 1)
                s[tuple(sl)] += dt(2 * w[d])
    rest[-1] = s
    acc = None
    for d in range(rank):
        up = list(where)
        up[d] = slice(2, 2 + m[d])
        for t in (rest[d][where], rest[d][tuple(up)]):
            acc = t.copy() if acc is None else (acc + t).astype(dt)
    diag = np.zeros(shape, dtype)
    diag[where] = (acc + s[where]).astype(dt)
    return rest, diag


def flux_levels(steps, damp, dtype=np.float64, faces="neumann"):
    """mgcc_cases.flux_levels; faces may also be a (low, high) pair per dimension (the module then always has its diagonal
    field); -> (levels, texts, rests)"""
    if isinstance(faces, str):
        return cc.flux_levels(steps, damp, dtype, faces)
    dt = np.dtype(dtype).type
    levels, texts, rests = [], [], []
    for l, (m, w, axes) in enumerate(steps):
        shape = tuple(n + 2 for n in m)
        where = tuple(slice(1, 1 + n) for n in m)
        text = cc.flux_module(shape, dtype, diagonal=True)
        rest, diag = mixed_face_fields(m, dtype, faces, w)
        minv = np.full(shape, 0.0 if l == 0 else np.nan, dtype)
        minv[where] = (dt(damp) / diag[where]).astype(dt)
        L = rst.Level(rst.Operator(text, *rest), shape, where, minv, dtype)
        L.axes, L.weights = axes, w
        levels.append(L)
        texts.append(text)
        rests.append(rest)
    return levels, texts, rests


def star_s_module(shape, dtype=np.float64):
    """NeptuneIR text of @entry(out, u, s), bounds one cell in from every face: out = (2 rank * u - (the star neighbours, added
    in the order lower, upper per dimension)) + s * u.  With u = 0 outside Omega this is the flux form of mgcc_cases with unit
    coefficients when s = +1 per Dirichlet boundary face of the cell (the ghost mirrored with its sign flipped) and -1 per
    Neumann one (the ghost mirrored) -- two inputs whatever the rank, where the flux form of rank 3 with a diagonal has five,
    more than a lowered apply takes"""
    import monitor_cases as mc
    rank = len(shape)
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "x".join(["?"] * rank) + "x" + elem
    zero = [0] * rank
    body = [f"        %uc = neptune_ir.access %u0[{lst(zero)}] : !temp -> {elem}"]
    names = []
    for d in range(rank):
        for sgn, tag in ((-1, "m"), (1, "p")):
            off = list(zero)
            off[d] = sgn
            body.append(f"        %u{tag}{d} = neptune_ir.access %u0[{lst(off)}] : !temp -> {elem}")
            names.append(f"u{tag}{d}")
    body += [f"        %sg = neptune_ir.access %ks[{lst(zero)}] : !temp -> {elem}",
             f"        %wc = arith.constant {float(2 * rank)!r} : {elem}",
             f"        %n1 = arith.addf %{names[0]}, %{names[1]} : {elem}"]
    for i, nm in enumerate(names[2:], start=2):
        body.append(f"        %n{i} = arith.addf %n{i - 1}, %{nm} : {elem}")
    body += [f"        %t0 = arith.mulf %wc, %uc : {elem}", f"        %t1 = arith.subf %t0, %n{len(names) - 1} : {elem}",
             f"        %t2 = arith.mulf %sg, %uc : {elem}", f"        %t3 = arith.addf %t1, %t2 : {elem}",
             f"        neptune_ir.yield %t3 : {elem}"]
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(zero)}], ub = [{lst(shape)}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst([1] * rank)}], ub = [{lst([n - 1 for n in shape])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>, %in1: memref<{mr}>) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu = neptune_ir.wrap %in : memref<{mr}> -> !field", "    %u = neptune_ir.load %fu : !field -> !temp",
           f"    %fs = neptune_ir.wrap %in1 : memref<{mr}> -> !field", "    %s = neptune_ir.load %fs : !field -> !temp",
           "    %r = neptune_ir.apply(%u, %s) attributes {bounds = #bi} : (!temp, !temp) -> !temp {",
           "      ^bb0(" + ", ".join([f"%i{d}: index" for d in range(rank)] + ["%u0: !temp", "%ks: !temp"]) + "):"] + body + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def star_levels(steps, damp, dtype=np.float64, faces="dirichlet"):
    """flux_levels for star_s_module, every pair halving every dimension (unit weights): rest = [s], minv = damp / (2 rank + s) on
    Omega, 0 outside on level 0 and NaN on the coarser ones; -> (levels, texts, rests)"""
    dt = np.dtype(dtype).type
    levels, texts, rests = [], [], []
    for l, (m, w, axes) in enumerate(steps):
        rank = len(m)
        assert all(v == 1.0 for v in w) and (l == len(steps) - 1 or tuple(axes) == tuple(range(rank))), (w, axes)
        pairs = [(faces, faces)] * rank if isinstance(faces, str) else faces
        shape = tuple(n + 2 for n in m)
        where = tuple(slice(1, 1 + n) for n in m)
        s = np.zeros(shape, dtype)
        for d in range(rank):
            for edge, kind in zip((1, m[d]), pairs[d]):
                sl = list(where)
                sl[d] = slice(edge, edge + 1)
                s[tuple(sl)] += dt(1.0 if kind == "dirichlet" else -1.0)
        text = star_s_module(shape, dtype)
        minv = np.full(shape, 0.0 if l == 0 else np.nan, dtype)
        minv[where] = (dt(damp) / (dt(2 * rank) + s[where]).astype(dt)).astype(dt)
        L = rst.Level(rst.Operator(text, s), shape, where, minv, dtype)
        L.axes, L.weights = axes, w
        levels.append(L)
        texts.append(text)
        rests.append([s])
    return levels, texts, rests


def problem(levels, faces, dtype=np.float64):
    """x0 = 0 and a hashed b, made compatible when every face is a Neumann one"""
    L0 = levels[0]
    x0, b = mgc.problem_fields(L0.shape, L0.where, dtype)
    all_neumann = faces == "neumann" or (not isinstance(faces, str) and all(v == "neumann" for f in faces for v in f))
    return x0, (cc.compatible(b, L0.where) if all_neumann else b)
