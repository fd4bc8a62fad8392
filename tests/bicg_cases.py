"""Operator and NumPy references of the BiCGStab tests.

The operator is a 7-point first-order upwind advection-diffusion operator with a reaction term:
    A(u)<p> = (6 + c0 + c1 + c2 + sigma) * u<p> - sum_d (1 + c_d) * u<p - e_d> - sum_d u<p + e_d>
on the interior, copy-through on the rim, with c = (4, 2, 1) and sigma = 1: centre weight 14, lower neighbours 5, 3, 2, upper
neighbours 1.  Every constant is a small integer, so the coefficients are exact in f32 and f64.  It is not symmetric (the
lower and upper weights differ), diagonally dominant by sigma, and plain CG diverges on it (tests/test_bicg_host.py pins both).

ONE association order, in the module text and in numpy_operator alike:
    m_d = (1 + c_d) * u<p - e_d>                     three products
    s   = ((((m_0 + m_1) + m_2) + u<p + e_0>) + u<p + e_1>) + u<p + e_2>      left to right
    A(u)<p> = (14 * u<p>) - s                         one product, one subtraction
every operation rounded once in the element type.  At rank 1 and 2 the same with c = C_ADV[:rank]: rank products, s summed in
the same order over the dimensions there are, centre weight 2 * rank + sum(c) + sigma (9 at rank 2, 7 at rank 1).

Everything else follows the normative definition of neptune_hip_bicgstab_solve (include/neptune_hip.h) the way cg_cases
follows neptune_hip_cg_solve's: arithmetic in the element type, one rounding per operation (numpy never fuses), the operator
itself from the oracle."""
import math

import numpy as np

import cg_cases as cc
import helpers
import monitor_cases as mc

C_ADV = (4.0, 2.0, 1.0)
SIGMA = 1.0


def bicg_module(shape, dtype=np.float64, origin=None, bounds=None):
    """NeptuneIR text of @entry(out, in): out = A(in) as described above (pcg_cases.pcg_module's frame: box
    [origin, origin + shape), origin 0 by default; `bounds` logical, by default one cell in from every face); rank 1 to 3"""
    rank = len(shape)
    assert 1 <= rank <= 3
    origin = [0] * rank if origin is None else [int(x) for x in origin]
    if bounds is None:
        bounds = ([o + 1 for o in origin], [o + n - 1 for o, n in zip(origin, shape)])
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "x".join(["?"] * rank) + "x" + elem
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    zero = [0] * rank
    acc = [f"        %c = neptune_ir.access %a[{lst(zero)}] : !temp -> {elem}"]
    for d in range(rank):
        for sgn, tag in ((-1, "m"), (1, "p")):
            off = list(zero)
            off[d] = sgn
            acc.append(f"        %n{d}{tag} = neptune_ir.access %a[{lst(off)}] : !temp -> {elem}")
    ops = [f"        %wc = arith.constant {centre_weight(rank)!r} : {elem}"]
    for d in range(rank):
        ops += [f"        %w{d} = arith.constant {1.0 + C_ADV[d]!r} : {elem}",
                f"        %m{d} = arith.mulf %w{d}, %n{d}m : {elem}"]
    # s = m_0 + ... + m_(rank-1) + u<p + e_0> + ... + u<p + e_(rank-1)>, left to right
    terms = [f"m{d}" for d in range(rank)] + [f"n{d}p" for d in range(rank)]
    prev = terms[0]
    for t, nm in enumerate(terms[1:]):
        ops.append(f"        %s{t} = arith.addf %{prev}, %{nm} : {elem}")
        prev = f"s{t}"
    ops += [f"        %t0 = arith.mulf %wc, %c : {elem}",
            f"        %t1 = arith.subf %t0, %{prev} : {elem}", f"        neptune_ir.yield %t1 : {elem}"]
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(origin)}], ub = [{lst([o + n for o, n in zip(origin, shape)])}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst(bounds[0])}], ub = [{lst(bounds[1])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu   = neptune_ir.wrap %in : memref<{mr}> -> !field",
           "    %u    = neptune_ir.load %fu : !field -> !temp",
           "    %r = neptune_ir.apply(%u) attributes {bounds = #bi} : (!temp) -> !temp {",
           f"      ^bb0({idx}, %a: !temp):"] + acc + ops + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def centre_weight(rank):
    """2 * rank + c_0 + ... + c_(rank-1) + sigma: 14 at rank 3, 9 at rank 2, 7 at rank 1"""
    return 2.0 * rank + sum(C_ADV[:rank]) + SIGMA


def numpy_operator(u: np.ndarray, origin=None, bounds=None) -> np.ndarray:
    """the operator restated in numpy, in the association order fixed above, at rank 1 to 3 with c = C_ADV[:rank]; origin and
    bounds (logical) as bicg_module's"""
    dt = u.dtype.type
    shape, rank = u.shape, u.ndim
    origin = [0] * rank if origin is None else list(origin)
    if bounds is None:
        bounds = ([o + 1 for o in origin], [o + n - 1 for o, n in zip(origin, shape)])
    where = mc.inside_slices(shape, origin, bounds)

    def nb(ax, sg):
        sl = list(where)
        sl[ax] = slice(where[ax].start + sg, where[ax].stop + sg)
        return u[tuple(sl)]
    m = [(dt(1.0 + C_ADV[d]) * nb(d, -1)).astype(dt) for d in range(rank)]
    s = m[0]
    for d in range(1, rank):
        s = (s + m[d]).astype(dt)
    for d in range(rank):
        s = (s + nb(d, 1)).astype(dt)
    out = u.copy()
    out[where] = ((dt(centre_weight(rank)) * u[where]).astype(dt) - s).astype(dt)
    return out


Operator = cc.Operator     # the oracle's A for one module text: q = A(p) into a fresh array


def _sum(terms: np.ndarray):
    return terms.dtype.type(np.sum(terms, dtype=terms.dtype))


def _alpha(dt, rho, rv):
    return dt(0) if (rho == 0 or rv == 0) else dt(rho / rv)


def _omega(dt, ts, tt):
    return dt(0) if tt == 0 else dt(ts / tt)


def _beta(dt, rho, rv, omega, rho_new, alpha):
    if rho == 0 or rv == 0 or omega == 0:
        return dt(0)
    return dt(dt(rho_new / rho) * dt(alpha / omega))


def setup(A, x, b, where):
    """the definition's set-up: -> (r, rh, p, rr0 as (value, bound)); rho_0 is rr_0"""
    dt = x.dtype.type
    v = A(x)
    r = np.zeros_like(x)
    r[where] = (b[where] - v[where]).astype(dt)
    return r, r.copy(), r.copy(), cc.dot_terms(r, r, where)


def _half_steps(dt, A, x, r, rh, p, v, alpha, scalars_of_t):
    """steps 2 - 5 of one iteration given v = A(p) and alpha; scalars_of_t(t, s) -> (ts, tt).  -> the new x and r, then s,
    t and omega"""
    s = (r - (alpha * v).astype(dt)).astype(dt)
    t = A(s)
    ts, tt = scalars_of_t(t, s)
    omega = _omega(dt, ts, tt)
    x = ((x + (alpha * p).astype(dt)).astype(dt) + (omega * s).astype(dt)).astype(dt)
    r = (s - (omega * t).astype(dt)).astype(dt)
    return x, r, s, t, omega


def _direction(dt, r, p, v, beta, omega):
    return (r + (beta * (p - (omega * v).astype(dt)).astype(dt)).astype(dt)).astype(dt)


def numpy_bicgstab(A, x0, b, where, iters, full=False):
    """the recurrences of the definition with numpy's own sums: -> the r . r sequence [rr_0, rr_1, ...] (floats), for the stop
    tests and the convergence checks; full=True: -> (seq, x, r, p, rr0, trace rows) as a device would report them"""
    dt = x0.dtype.type
    x = x0.copy()
    r, rh, p, _ = setup(A, x, b, where)
    rho = rr0 = _sum((r * r).astype(dt))
    seq = [float(rr0)]
    trace = []
    for _ in range(iters):
        v = A(p)
        rv = _sum((rh * v).astype(dt))
        alpha = _alpha(dt, rho, rv)
        got = {}

        def scalars(t, s):
            got["ts"] = _sum((t[where] * s[where]).astype(dt))
            got["tt"] = _sum((t * t).astype(dt))
            return got["ts"], got["tt"]
        x, r, s, t, omega = _half_steps(dt, A, x, r, rh, p, v, alpha, scalars)
        rho_new = _sum((rh * r).astype(dt))
        rr_new = _sum((r * r).astype(dt))
        beta = _beta(dt, rho, rv, omega, rho_new, alpha)
        p = _direction(dt, r, p, v, beta, omega)
        trace.append((rv, got["ts"], got["tt"], rho_new, rr_new))
        rho = rho_new
        seq.append(float(rr_new))
    if full:
        return seq, x, r, p, rr0, np.array(trace, dtype=x0.dtype).reshape(-1, 5)
    return seq


def replay(A, x0, b, where, rr0, trace):
    """The definition's recurrences driven by the DEVICE's scalars: iteration k takes alpha_k = rho_k / rv_k,
    omega_k = ts_k / tt_k and beta_k = (rho_(k+1) / rho_k) * (alpha_k / omega_k) from rho_0 = rr_0 and the trace rows
    (rv_k, ts_k, tt_k, rho_(k+1), rr_(k+1)), each division and the product rounded once in the element type, and v, t from the
    oracle's operator.  -> (x, r, p, checks), checks[k] = the five (terms' sum, bound) pairs of rv, ts, tt, rho' and rr' of the
    replay's own fields, for comparison with the traced scalars.  Whatever order the device summed in, the fields it holds
    must be these bit for bit."""
    dt = x0.dtype.type
    x = x0.copy()
    r, rh, p, _ = setup(A, x, b, where)
    rho = dt(rr0)
    checks = []
    everywhere = tuple(slice(None) for _ in x.shape)
    for k in range(len(trace)):
        rv, ts, tt, rho_new = (dt(trace[k][c]) for c in range(4))
        v = A(p)
        rv_ref = cc.dot_terms(rh, v, everywhere)
        alpha = _alpha(dt, rho, rv)
        refs = {}

        def scalars(t, s):
            refs["ts"] = cc.dot_terms(t, s, where)
            refs["tt"] = cc.dot_terms(t, t, everywhere)
            return ts, tt
        x, r, s, t, omega = _half_steps(dt, A, x, r, rh, p, v, alpha, scalars)
        checks.append((rv_ref, refs["ts"], refs["tt"], cc.dot_terms(rh, r, everywhere), cc.dot_terms(r, r, everywhere)))
        beta = _beta(dt, rho, rv, omega, rho_new, alpha)
        p = _direction(dt, r, p, v, beta, omega)
        rho = rho_new
    return x, r, p, checks


def numpy_cg_on(A, x0, b, where, iters):
    """plain CG's recurrence (cg_cases.numpy_cg) on any operator: the r . r sequence"""
    return cc.numpy_cg(A, x0, b, where, iters)


def stop_points(seq, upto):
    """BiCGStab's r . r is not monotone, so the stop tests pick their iterations from the numpy sequence: the indices
    1 <= k <= upto at which rr_k is below half the minimum of ALL earlier values; -> [(k, tol2)] with the threshold at the
    geometric mean of rr_k and that earlier minimum (a factor >= sqrt(2) from both, and no earlier value is below it)"""
    out = []
    for k in range(1, min(upto, len(seq) - 1) + 1):
        low = min(seq[:k])
        if seq[k] * 2.0 <= low and seq[k] > 0:
            out.append((k, math.sqrt(seq[k] * low)))
    return out


def expected_stop(seq, check_every, max_iters, tol2):
    return cc.expected_stop(seq, check_every, max_iters, tol2)


class Problem:
    """one test problem, built once and left unchanged: shape, dtype, module text, the oracle's operator, Omega, b, x0.
    origin: the logical lower corner of the fields' box (default 0); bounds: logical (default one cell in from every face);
    `where` is Omega in physical indices."""

    def __init__(self, shape, dtype, rim=False, origin=None, bounds=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.origin = tuple([0] * len(shape) if origin is None else [int(o) for o in origin])
        if bounds is None:
            bounds = ([o + 1 for o in self.origin], [o + n - 1 for o, n in zip(self.origin, shape)])
        self.text = bicg_module(shape, dtype, origin, bounds)
        self.A = Operator(self.text)
        self.bounds = bounds
        self.where = mc.inside_slices(shape, self.origin, bounds)
        self.b = helpers.hash_field(shape, dtype, seed=71)
        self.x0 = helpers.hash_field(shape, dtype, seed=72) if rim else np.zeros(shape, dtype)
        for a in (self.b, self.x0):
            a.setflags(write=False)
