"""Operator and NumPy references of the Jacobi-preconditioned conjugate-gradient tests.

The operator is a reaction-diffusion star with a coefficient field:
    A(u)<p> = (d + w<p>) * u<p> - (sum of the 2 * rank star neighbours of u at p)   on the interior, copy-through on the rim,
d = 4 * rank, w = input 1, read at the centre only.  w is drawn per cell from {0, 16, 256, 4096} by the hash of
helpers.hash_field: all values are dyadic, so (d + w) * 1 is exact in f32 and f64 and the diagonal d + w is known exactly.
With zero rim values A is symmetric positive definite; its diagonal spans 12 .. 4108 in 3-D, so plain CG needs about four
times the iterations of the diagonally preconditioned one (tests/test_pcg_host.py pins that).

Everything here follows the normative definition of neptune_hip_pcg_solve (include/neptune_hip.h) the way cg_cases follows
neptune_hip_cg_solve's: arithmetic in the element type, two roundings per update, z = minv * r rounded once, the operator
itself from the oracle."""
import itertools

import numpy as np

import cg_cases as cc
import helpers
import monitor_cases as mc

W_VALUES = (0.0, 16.0, 256.0, 4096.0)


def pcg_module(shape, dtype=np.float64, origin=None, bounds=None):
    """NeptuneIR text of @entry(out, in, in1): out = A(in) with w = in1 as described above (monitor_cases.star_module's
    frame: box [origin, origin + shape), origin 0 by default; `bounds` logical, by default one cell in from every face)"""
    rank = len(shape)
    origin = [0] * rank if origin is None else [int(x) for x in origin]
    if bounds is None:
        bounds = ([o + 1 for o in origin], [o + n - 1 for o, n in zip(origin, shape)])
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "x".join(["?"] * rank) + "x" + elem
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    zero = [0] * rank
    acc = [f"        %c = neptune_ir.access %a[{lst(zero)}] : !temp -> {elem}",
           f"        %wv = neptune_ir.access %o[{lst(zero)}] : !temp -> {elem}"]
    names = []
    for d in range(rank):
        for sgn, tag in ((-1, "m"), (1, "p")):
            off = list(zero)
            off[d] = sgn
            names.append(f"n{d}{tag}")
            acc.append(f"        %{names[-1]} = neptune_ir.access %a[{lst(off)}] : !temp -> {elem}")
    ops = [f"        %wc = arith.constant {float(4 * rank)!r} : {elem}", f"        %ws = arith.constant -1.0 : {elem}"]
    prev = names[0]
    for t, nm in enumerate(names[1:]):
        ops.append(f"        %s{t} = arith.addf %{prev}, %{nm} : {elem}")
        prev = f"s{t}"
    ops += [f"        %dw = arith.addf %wc, %wv : {elem}", f"        %t0 = arith.mulf %dw, %c : {elem}",
            f"        %t1 = arith.mulf %ws, %{prev} : {elem}", f"        %t2 = arith.addf %t0, %t1 : {elem}",
            f"        neptune_ir.yield %t2 : {elem}"]
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(origin)}], ub = [{lst([o + n for o, n in zip(origin, shape)])}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst(bounds[0])}], ub = [{lst(bounds[1])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>, %in1: memref<{mr}>) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu   = neptune_ir.wrap %in : memref<{mr}> -> !field",
           "    %u    = neptune_ir.load %fu : !field -> !temp",
           f"    %fv   = neptune_ir.wrap %in1 : memref<{mr}> -> !field",
           "    %v    = neptune_ir.load %fv : !field -> !temp",
           "    %r = neptune_ir.apply(%u, %v) attributes {bounds = #bi} : (!temp, !temp) -> !temp {",
           f"      ^bb0({idx}, %a: !temp, %o: !temp):"] + acc + ops + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def w_field(shape, dtype=np.float64, seed=73, values=W_VALUES):
    """one of `values` per cell, chosen by the f64 hash of the cell (the same choice for both element types)"""
    h = helpers.hash_field(shape, np.float64, seed=seed)                 # in [-1, 1)
    pick = np.clip(np.floor((h + 1.0) * (len(values) / 2.0)).astype(np.int64), 0, len(values) - 1)
    return np.asarray(values, dtype)[pick]


def diagonal(w: np.ndarray, where):
    """the exact diagonal of A on Omega (any part of apply.bounds), +0 elsewhere"""
    d = np.zeros_like(w)
    d[where] = (w.dtype.type(4 * w.ndim) + w[where]).astype(w.dtype)
    return d


def minv_of(diag: np.ndarray, where):
    """jacobi_minv's field: 1 / diag (one division) on Omega, 1 elsewhere"""
    m = np.ones_like(diag)
    m[where] = (diag.dtype.type(1) / diag[where]).astype(diag.dtype)
    return m


class Operator:
    """the oracle's A for one module text and one coefficient field: q = A(p) into a fresh array"""

    def __init__(self, text, w):
        self.module = helpers.oracle.Module.parse(text)
        self.w = w

    def __call__(self, u: np.ndarray) -> np.ndarray:
        out = np.zeros_like(u)
        self.module.call("entry", out, u, self.w)
        return out


def probe_diagonal(A, shape, dtype, where, reach=1):
    """apply.operator_diagonal's procedure on any callable operator: coloured unit vectors with stride 2 * reach + 1 per
    dimension, 1 on the cells of Omega of one colour and 0 elsewhere, one application per colour, the result copied at
    exactly those cells"""
    lo = [s.start for s in where]
    hi = [s.stop for s in where]
    s = 2 * reach + 1
    diag = np.zeros(shape, dtype)
    for colour in itertools.product(*[range(min(s, h - l)) for l, h in zip(lo, hi)]):
        cells = tuple(slice(l + c, h, s) for l, h, c in zip(lo, hi, colour))
        probe = np.zeros(shape, dtype)
        probe[cells] = 1
        diag[cells] = A(probe)[cells]
    return diag


def z_dot_terms(r: np.ndarray, minv: np.ndarray, where):
    """-> (sum, bound) of the terms r * (minv * r) over `where`: z rounded once, then the product, as cg_cases.dot_terms"""
    dt = r.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        z = (minv * r).astype(dt)
    return cc.dot_terms(r, z, where)


def _sum(terms: np.ndarray):
    return terms.dtype.type(np.sum(terms, dtype=terms.dtype))


def setup(A, x, b, minv, where):
    """the definition's set-up: -> (r, p, rz0 as (value, bound), rr0 as (value, bound))"""
    dt = x.dtype.type
    q = A(x)
    r = np.zeros_like(x)
    r[where] = (b[where] - q[where]).astype(dt)
    p = np.zeros_like(x)
    p[where] = (minv[where] * r[where]).astype(dt)
    return r, p, z_dot_terms(r, minv, where), cc.dot_terms(r, r, where)


def numpy_pcg(A, x0, b, minv, where, iters):
    """the recurrences of the definition with numpy's own sums: -> the r . r sequence [rr_0, rr_1, ...] (floats), for the stop
    tests and the convergence checks"""
    dt = x0.dtype.type
    x = x0.copy()
    r, p, _, _ = setup(A, x, b, minv, where)
    z = (minv * r).astype(dt)
    rz = _sum((r * z).astype(dt))
    seq = [float(_sum((r * r).astype(dt)))]
    for _ in range(iters):
        q = A(p)
        pq = _sum((q[where] * p[where]).astype(dt))
        broken = rz == 0 or pq == 0
        alpha = dt(0) if broken else dt(rz / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        z = (minv * r).astype(dt)
        rz_new = _sum((r * z).astype(dt))
        beta = dt(0) if broken else dt(rz_new / rz)
        p = (z + (beta * p).astype(dt)).astype(dt)
        rz = rz_new
        seq.append(float(_sum((r * r).astype(dt))))
    return seq


def replay(A, x0, b, minv, where, rz0, trace):
    """The definition's recurrences driven by the DEVICE's scalars: iteration k takes alpha_k = rz_k / pq_k and
    beta_k = rz_(k+1) / rz_k from rz_0 and the trace rows (pq_k, rz_(k+1), rr_(k+1)), each one division in the element type,
    and q from the oracle's operator.  -> (x, r, p, checks), checks[k] = the (terms' sum, bound) pairs of pq, rz' and rr' of the
    replay's own fields, for comparison with the traced scalars."""
    dt = x0.dtype.type
    x = x0.copy()
    r, p, _, _ = setup(A, x, b, minv, where)
    rz = dt(rz0)
    checks = []
    everywhere = tuple(slice(None) for _ in x.shape)
    for k in range(len(trace)):
        pq, rz_new = dt(trace[k][0]), dt(trace[k][1])
        q = A(p)
        pq_ref = cc.dot_terms(q, p, where)
        broken = rz == 0 or pq == 0
        alpha = dt(0) if broken else dt(rz / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        z = (minv * r).astype(dt)
        checks.append((pq_ref, cc.dot_terms(r, z, everywhere), cc.dot_terms(r, r, everywhere)))
        beta = dt(0) if broken else dt(rz_new / rz)
        p = (z + (beta * p).astype(dt)).astype(dt)
        rz = rz_new
    return x, r, p, checks


class Problem:
    """one test problem, built once and left unchanged: shape, dtype, module text, w, the oracle's operator, Omega, b, x0,
    the exact diagonal and the Jacobi minv.  origin: the logical lower corner of the fields' box (default 0); bounds: logical
    (default one cell in from every face); `where` is Omega in physical indices."""

    def __init__(self, shape, dtype, rim=False, w_values=W_VALUES, origin=None, bounds=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.origin = tuple([0] * len(shape) if origin is None else [int(o) for o in origin])
        if bounds is None:
            bounds = ([o + 1 for o in self.origin], [o + n - 1 for o, n in zip(self.origin, shape)])
        self.text = pcg_module(shape, dtype, origin, bounds)
        self.w = w_field(shape, dtype, values=w_values)
        self.A = Operator(self.text, self.w)
        self.bounds = bounds
        self.where = mc.inside_slices(shape, self.origin, bounds)
        self.b = helpers.hash_field(shape, dtype, seed=71)
        self.x0 = helpers.hash_field(shape, dtype, seed=72) if rim else np.zeros(shape, dtype)
        self.diag = diagonal(self.w, self.where)
        self.minv = minv_of(self.diag, self.where)
        for a in (self.w, self.b, self.x0, self.diag, self.minv):
            a.setflags(write=False)


# The iterations over which the GPU stop tests place their thresholds: numpy_pcg's r . r falls by at least 2x per iteration
# over these, before the rounding floor of the element type (test_pcg_host.py checks it on the CPU).
STOP_ITERS = {np.float64: 10, np.float32: 6}
