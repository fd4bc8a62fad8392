"""The problems of the multigrid tests: module texts, hierarchies and fields; the restatement they run on is
mg_restatement's.

The operator is the star of monitor_cases.star_module with centre weight 2 * rank and side weight -1 -- the unscaled Poisson
operator, one module per level shape --, rscale = 4, and damped-Jacobi weights minv = omega / (2 * rank) on Omega."""
import numpy as np

import helpers
import mg_restatement as rst
import monitor_cases as mc


def mg_module(shape, dtype=np.float64):
    """NeptuneIR text of @entry(out, in): out = 2 rank * in - (sum of the star neighbours) one cell in from every face"""
    return mc.star_module(shape, dtype, centre=float(2 * len(shape)), side=-1.0)


# ---------------------------------------------------------------- hierarchies of the star operator
def level_shapes(omega, levels, rims=None):
    """box shapes and Omega slices of `levels` nested levels starting from interior extents `omega`; rims: per level a
    (lower, upper) pair of per-dimension rim widths (default one cell everywhere, what mg_module's bounds need)"""
    out, m = [], [int(v) for v in omega]
    for l in range(levels):
        lo, up = rims[l] if rims else ([1] * len(m), [1] * len(m))
        shape = tuple(a + n + b for a, n, b in zip(lo, m, up))
        where = tuple(slice(a, a + n) for a, n in zip(lo, m))
        out.append((shape, where))
        if l + 1 < levels:
            assert all(n % 2 == 1 and n >= 3 for n in m), m
            m = [(n - 1) // 2 for n in m]
    return out


def minv_field(shape, where, dtype, omega, outside=np.nan):
    """omega / (2 rank) on Omega (one division in the element type), `outside` elsewhere: NaN proves the rim is never used"""
    dt = np.dtype(dtype).type
    m = np.full(shape, outside, dtype)
    m[where] = dt(dt(omega) / dt(2 * len(shape)))
    return m


def star_levels(omega, n_levels, dtype, omega_damp, texts=None):
    """restatement levels of the star operator on whole-interior boxes (rim of one cell); -> (levels, module texts)"""
    shapes = level_shapes(omega, n_levels)
    texts = texts or [mg_module(shape, dtype) for shape, _ in shapes]
    levels = [rst.Level(rst.Operator(text), shape, where, minv_field(shape, where, dtype, omega_damp), dtype)
              for text, (shape, where) in zip(texts, shapes)]
    return levels, texts


def problem_fields(shape, where, dtype, rim=False, seed=91):
    """b (hashed) and x0: zeros, or hashed non-zero Dirichlet values on the rim with zeros inside"""
    b = helpers.hash_field(shape, dtype, seed=seed)
    x0 = np.zeros(shape, dtype)
    if rim:
        x0 = helpers.hash_field(shape, dtype, seed=seed + 1)
        x0[where] = 0
    return x0, b
