"""The NumPy restatement of the linear prolongation on cell-centred pairs, on mgcc_cases.

Along a halved dimension the fine cell i has j = i / 2 and the neighbour n = j - 1 (even i) or j + 1 (odd i):
    p = 0.75 * e[j],  s = 0.25 * v,  t = p + s,    v = e[n], or outside [0, m_c) the ghost +e[j] (EVEN) / -e[j] (ODD)
in the element type with one `.astype(dt)` per operation, the last dimension first, kept dimensions skipped.  e is the
intermediate after the dimensions already done: the ghosts come from padding THAT array with +- its edge, which is what
include/neptune_hip.h defines.

A level carries `.axes` as everywhere else; a pair that prolongs linearly carries a Linear(axes, rim) -- an
mgcc_cases.Halved, so the restriction stays mgcc_cases' averaging one -- whose .rim[d] = (low rule, high rule) per field
dimension.  prolong_add dispatches on that marker and hands everything else to mgcc_cases.prolong_add.  cycle, run and
rr_sequence are mgsemi_cases' own functions re-bound to this module's namespace, as mgcc_cases re-binds them; lines_run is
mgfuzz_cases' composed cycle (line stages per level) re-bound the same way.  Nothing of them is written twice."""
import types

import numpy as np

import mg_cases as mgc
import mgcc_cases as cc
import mgfuzz_cases as fz
import mgsemi_cases as sc
from mgcc_cases import Halved

EVEN, ODD = 0, 1            # NEPTUNE_HIP_MG_RIM_EVEN / _ODD
RULE = {"neumann": EVEN, "dirichlet": ODD}
expected_stop = mgc.expected_stop
tol_between = mgc.tol_between
restrict = cc.restrict      # a Linear is a Halved: the averaging restriction


class Linear(Halved):
    """the dimensions halved between a level and the next one, prolonged linearly; .rim[d] = (low, high) rule of dimension d"""

    def __new__(cls, axes, rim):
        self = super().__new__(cls, axes)
        self.rim = tuple((int(lo), int(hi)) for lo, hi in rim)
        assert all(v in (EVEN, ODD) for pair in self.rim for v in pair)
        return self


def rim_of(faces, rank):
    """((low, high) rule per dimension) for faces = "neumann" / "dirichlet" or a (low, high) pair of them per dimension"""
    if isinstance(faces, str):
        faces = [(faces, faces)] * rank
    assert len(faces) == rank
    return tuple((RULE[lo], RULE[hi]) for lo, hi in faces)


def complement(rim):
    return tuple((1 - lo, 1 - hi) for lo, hi in rim)


# ---------------------------------------------------------------- the prolongation
def _linear(e, axis, rule_lo, rule_hi):
    """m -> 2 m cells along `axis`: fine 2 j takes 0.75 e[j] + 0.25 e[j - 1], fine 2 j + 1 takes 0.75 e[j] + 0.25 e[j + 1], e
    padded with + (EVEN) or - (ODD) its own edge"""
    dt = e.dtype.type
    m = e.shape[axis]
    take = lambda a, idx: np.take(a, idx, axis=axis)
    first, last = take(e, [0]), take(e, [m - 1])
    with np.errstate(invalid="ignore", over="ignore"):
        padded = np.concatenate([-first if rule_lo == ODD else first, e, -last if rule_hi == ODD else last], axis=axis)
        p = (dt(0.75) * e).astype(dt)
        sm = (dt(0.25) * take(padded, np.arange(0, m))).astype(dt)
        sp = (dt(0.25) * take(padded, np.arange(2, m + 2))).astype(dt)
        even = (p + sm).astype(dt)
        odd = (p + sp).astype(dt)
    shape = list(e.shape)
    shape[axis] = 2 * m
    out = np.empty(shape, e.dtype)
    sl = [slice(None)] * e.ndim
    sl[axis] = slice(0, None, 2)
    out[tuple(sl)] = even
    sl[axis] = slice(1, None, 2)
    out[tuple(sl)] = odd
    return out


def prolong_add_linear(x_c, where_c, x_f, where_f, axes, rim):
    """-> a new x_f: x_f + P(x_c) on the fine Omega, P linear along `axes` by the rules rim[d] = (low, high); every other cell
    keeps its bits; nothing outside where_c is read"""
    dt = x_f.dtype.type
    e = x_c[where_c]
    for axis in reversed(range(e.ndim)):
        if axis in axes:
            e = _linear(e, axis, *rim[axis])
    out = x_f.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[where_f] = (x_f[where_f] + e).astype(dt)
    return out


def prolong_add(x_c, where_c, x_f, where_f, axes):
    if isinstance(axes, Linear):
        return prolong_add_linear(x_c, where_c, x_f, where_f, axes, axes.rim)
    return cc.prolong_add(x_c, where_c, x_f, where_f, axes)


# ---------------------------------------------------------------- the cycle and the solve, re-bound
def _rebound(fn, namespace=None):
    out = types.FunctionType(fn.__code__, globals() if namespace is None else namespace, fn.__name__, fn.__defaults__)
    out.__doc__ = fn.__doc__
    return out


cycle = _rebound(sc.cycle)
run = _rebound(sc.run)
rr_sequence = _rebound(sc.rr_sequence)

# mgfuzz_cases' composed cycle (a level may carry .stages) calls cc.restrict / cc.prolong_add: its globals with `cc` = this
# module's two transfers
_composed = dict(vars(fz))
_composed["cc"] = types.SimpleNamespace(restrict=restrict, prolong_add=prolong_add)
for _name in ("descend", "cycle", "run"):
    _composed[_name] = _rebound(getattr(fz, _name), _composed)
lines_run = _composed["run"]


# ---------------------------------------------------------------- hierarchies
def linear_steps(steps, rim, only=None):
    """mgcc_cases' steps [(extents, weights, axes)] with every Halved pair (or the pairs listed in `only`) made Linear"""
    out = []
    for l, (m, w, axes) in enumerate(steps):
        if isinstance(axes, Halved) and len(axes) and (only is None or l in only):
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
        L = mgc.Level(mgc.Operator(text, *rest), shape, where, minv, dtype)
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
        L = mgc.Level(mgc.Operator(text, s), shape, where, minv, dtype)
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
