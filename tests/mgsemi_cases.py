"""The problems of semi-coarsened multigrid: hierarchies whose levels carry `.axes`, the dimensions coarsened
towards the next level (m_fine = 2 m_coarse + 1); every other dimension is kept (m_fine = m_coarse, the identity: no operation,
no rounding).  mg_restatement's transfers, cycle and MGCG run on them.

plan() restates the rule of neptune_hip.multigrid.coarsening_plan for operators -sum_d w_d u_dd on unscaled stencils with
rscale = 4; plan_levels builds the restatement's levels and module texts from it (mgcg_cases.aniso_module with the
per-level weights, damped-Jacobi weights damp / diagonal on Omega)."""
import numpy as np

import mg_restatement as rst
import mgcg_cases as mg


# ---------------------------------------------------------------- hierarchies
def next_level(extents, weights, axes):
    """the plan rule's step: (m - 1) / 2 and w on a coarsened dimension, m and 4 w on a kept one"""
    assert axes and all(extents[d] % 2 == 1 and extents[d] >= 3 for d in axes), (extents, axes)
    return (tuple((m - 1) // 2 if d in axes else m for d, m in enumerate(extents)),
            tuple(w if d in axes else 4.0 * w for d, w in enumerate(weights)))


def plan(extents, weights, threshold=0.5, max_levels=16):
    """the rule of multigrid.coarsening_plan, restated: -> [(extents, weights, axes)], axes = () on the last level"""
    m, w, out = tuple(int(v) for v in extents), tuple(float(v) for v in weights), []
    while True:
        can = [d for d, v in enumerate(m) if v % 2 == 1 and v >= 3]
        if not can or len(out) + 1 >= max_levels:
            out.append((m, w, ()))
            return out
        top = max(w[d] for d in can)
        axes = tuple(d for d in can if w[d] >= threshold * top)
        out.append((m, w, axes))
        m, w = next_level(m, w, axes)


def with_axes(extents, weights, axes_per_pair):
    """[(extents, weights, axes)] for a hierarchy given by the dimensions coarsened per pair, weights by the plan rule"""
    m, w, out = tuple(int(v) for v in extents), tuple(float(v) for v in weights), []
    for axes in axes_per_pair:
        out.append((m, w, tuple(axes)))
        m, w = next_level(m, w, tuple(axes))
    out.append((m, w, ()))
    return out


def build_levels(steps, damp, dtype, outside0=0.0):
    """restatement levels (whole-interior boxes, rim of one cell) and module texts for [(extents, weights, axes)]: the
    anisotropic star with the level's weights, minv = damp / diagonal on Omega; outside Omega level 0's minv is `outside0`
    (MGCG forms minv_0 * r on the whole box), the coarser levels' NaN (never read); -> (levels, texts)"""
    dt = np.dtype(dtype).type
    levels, texts = [], []
    for l, (m, w, axes) in enumerate(steps):
        shape = tuple(n + 2 for n in m)
        where = tuple(slice(1, 1 + n) for n in m)
        text = mg.aniso_module(shape, w, dtype)
        minv = np.full(shape, outside0 if l == 0 else np.nan, dtype)
        minv[where] = dt(dt(damp) / dt(2.0 * sum(w)))
        L = rst.Level(rst.Operator(text), shape, where, minv, dtype)
        L.axes, L.weights = axes, w
        levels.append(L)
        texts.append(text)
    return levels, texts


def plan_levels(omega, weights, damp, dtype=np.float64, threshold=0.5, max_levels=16, outside0=0.0):
    """restatement levels and module texts from the plan rule; -> (levels, texts)"""
    return build_levels(plan(omega, weights, threshold, max_levels), damp, dtype, outside0)


def full_levels(omega, weights, damp, dtype=np.float64, outside0=0.0):
    """the fully coarsened hierarchy of the same operator (every level the same weights), down to where an extent is even
    or below 3"""
    steps, m = [], tuple(omega)
    while all(v % 2 == 1 and v >= 3 for v in m):
        steps.append(tuple(range(len(m))))
        m = tuple((v - 1) // 2 for v in m)
    return build_levels(with_axes(omega, weights, steps), damp, dtype, outside0)
