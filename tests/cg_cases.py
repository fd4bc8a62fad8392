"""Operators and NumPy references of the conjugate-gradient tests.

The operator is the star of monitor_cases.star_module with centre weight d and side weight -1:
    A(u)<p> = d * u<p> - (sum of the 2 * rank * radius star neighbours of u at p)   on the interior, copy-through on the rim.
With d = 2 * (number of neighbours) -- 12 for the 7-point star, 24 for the radius-2 star -- and zero rim values (what the
solver's r and p carry) it is symmetric and its eigenvalues lie in (d / 2, 3 d / 2): positive definite, condition number at
most 3, so r . r falls by about an order of magnitude per iteration.

Everything here follows the normative definition of neptune_hip_cg_solve (include/neptune_hip.h): arithmetic in the element
type, two roundings per update (numpy never fuses), the operator itself from the oracle."""
import math

import numpy as np

import helpers
import monitor_cases as mc


def cg_module(shape, dtype=np.float64, origin=None, bounds=None, radius=1):
    """NeptuneIR text of @entry(out, in): out = A(in) as described above"""
    rank = len(shape)
    return mc.star_module(shape, dtype, origin, bounds, radius=radius, centre=float(4 * rank * radius), side=-1.0)


def interior(shape, radius=1):
    return ([radius] * len(shape), [n - radius for n in shape])


def dot_terms(fresh: np.ndarray, old: np.ndarray, where):
    """-> (D, bound): the terms fresh * old over `where`, each rounded once in the fields' element type, summed exactly
    (math.fsum); bound = 2 (n - 1) eps sum |t_i|, what any two summation orders of these n terms may differ by"""
    dt = fresh.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (fresh[where] * old[where]).astype(dt)
    flat = [float(t) for t in terms.ravel()]
    n = len(flat)
    if n == 0:
        return 0.0, 0.0
    return math.fsum(flat), 2.0 * (n - 1) * float(np.finfo(dt).eps) * math.fsum(abs(t) for t in flat)


class Operator:
    """the oracle's A for one module text: q = A(p) into a fresh array"""

    def __init__(self, text):
        self.module = helpers.oracle.Module.parse(text)

    def __call__(self, u: np.ndarray) -> np.ndarray:
        out = np.zeros_like(u)
        self.module.call("entry", out, u)
        return out


def _tree_free_sum(terms: np.ndarray) -> float:
    """the sum a device tree approximates: here numpy's pairwise sum in the element type (one order among many)"""
    return float(np.sum(terms, dtype=terms.dtype))


def setup(A, x, b, where):
    """the definition's set-up: -> (r, p, rr0 as (value, bound))"""
    dt = x.dtype.type
    q = A(x)
    r = np.zeros_like(x)
    r[where] = (b[where] - q[where]).astype(dt)
    return r, r.copy(), dot_terms(r, r, where)


def numpy_cg(A, x0, b, where, iters):
    """the recurrences of the definition with numpy's own sums: -> the r . r sequence [rr_0, rr_1, ...] (floats).  Used for
    the stop tests, whose thresholds sit a factor >= sqrt(2) away from every value of this sequence."""
    dt = x0.dtype.type
    x = x0.copy()
    r, p, _ = setup(A, x, b, where)
    rr = dt(_tree_free_sum((r * r).astype(dt)))
    seq = [float(rr)]
    for _ in range(iters):
        q = A(p)
        pq = dt(_tree_free_sum((q[where] * p[where]).astype(dt)))
        alpha = dt(0) if (rr == 0 or pq == 0) else dt(rr / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        rr_new = dt(_tree_free_sum((r * r).astype(dt)))
        beta = dt(0) if (rr == 0 or pq == 0) else dt(rr_new / rr)
        p = (r + (beta * p).astype(dt)).astype(dt)
        rr = rr_new
        seq.append(float(rr))
    return seq


def replay(A, x0, b, where, rr0, trace):
    """The definition's recurrences driven by the DEVICE's scalars: iteration k takes alpha_k = rr_k / pq_k and
    beta_k = rr_(k+1) / rr_k from rr_0 and the trace rows (pq_k, rr_(k+1)), each one division in the element type, and q
    from the oracle's operator.  -> (x, r, p, checks) where checks[k] = ((pq terms' sum, bound), (rr terms' sum, bound)) of the
    replay's own fields, for comparison with the traced scalars.  Whatever order the device summed in, the fields it holds
    must be these bit for bit."""
    dt = x0.dtype.type
    x = x0.copy()
    r, p, _ = setup(A, x, b, where)
    rr = dt(rr0)
    checks = []
    everywhere = tuple(slice(None) for _ in x.shape)
    for k in range(len(trace)):
        pq, rr_new = dt(trace[k][0]), dt(trace[k][1])
        q = A(p)
        pq_ref = dot_terms(q, p, where)
        alpha = dt(0) if (rr == 0 or pq == 0) else dt(rr / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        rr_ref = dot_terms(r, r, everywhere)
        beta = dt(0) if (rr == 0 or pq == 0) else dt(rr_new / rr)
        p = (r + (beta * p).astype(dt)).astype(dt)
        rr = rr_new
        checks.append((pq_ref, rr_ref))
    return x, r, p, checks


def expected_stop(seq, check_every, max_iters, tol2):
    """what the loop's definition gives on an r . r sequence: (iters_done, checks)"""
    if seq[0] <= tol2:
        return 0, 0
    done, checks = 0, 0
    while done < max_iters:
        done += min(check_every, max_iters - done)
        checks += 1
        if seq[done] <= tol2:
            break
    return done, checks


def tol_between(seq, a, b):
    """a threshold at the geometric mean of seq[a] and seq[b], which must differ by at least a factor of 2: two summation
    orders move r . r by at most 7e-14 (f64) / 5e-5 (f32) relative over 13 iterations, so the stop cannot hinge on rounding"""
    assert seq[b] * 2.0 <= seq[a], "precondition: consecutive check values differ by at least a factor of 2"
    return math.sqrt(seq[a] * seq[b])
