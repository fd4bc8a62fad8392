"""The problems of the transposed linear restriction on cell-centred pairs: a pair carries a
Transfers(axes, rim, prolong, restrict) -- the one rule array .rim[d] = (low rule, high rule) serves BOTH transfers,
.prolong = "constant" | "linear" and .restrict = "average" | "linear".  The operators and fields are mgcl_cases'; the
transfers, the cycle and MGCG are mg_restatement's."""
import numpy as np

import mg_restatement as rst
import mgcl_cases as cl
from mg_restatement import Transfers

flux_levels = cl.flux_levels
star_levels = cl.star_levels
problem = cl.problem


# ---------------------------------------------------------------- hierarchies
def transfer_steps(steps, rim, prolong="linear", restrict="linear", only=None):
    """mgcc_cases' steps [(extents, weights, axes)] with every Halved pair (or the pairs listed in `only`) made a
    Transfers(axes, rim, prolong, restrict)"""
    out = []
    for l, (m, w, axes) in enumerate(steps):
        if rst.pair_of(axes, len(m)).halved and len(axes) and (only is None or l in only):
            axes = Transfers(axes, rim, prolong, restrict)
        out.append((m, w, axes))
    return out


def mgcg_iterations(steps, faces, damp, sweeps, factor=1e-16, coarse_sweeps=8, dtype=np.float64, max_iters=60):
    """the iteration at which numpy_mgcg on flux_levels(steps, faces) first has r . r <= factor * rr_0, from x = 0 and
    mgcl_cases.problem's b"""
    levels, _, _ = flux_levels(steps, damp, dtype, faces)
    x0, b = problem(levels, faces, dtype)
    L0 = levels[0]
    terms = (b[L0.where] * b[L0.where]).astype(L0.dt)
    rr0 = float(np.sum(terms, dtype=terms.dtype))
    seq = rst.numpy_mgcg(levels, x0, b, max_iters, sweeps, coarse_sweeps, stop_at=factor * rr0)
    assert seq[-1] <= factor * seq[0], "not converged"
    return len(seq) - 1
