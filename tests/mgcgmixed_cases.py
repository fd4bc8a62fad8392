"""The problems of mixed-precision multigrid-preconditioned conjugate gradients (neptune_hip_mgcg_solve_mixed):
an f64 outer operator around f32 levels, and their device side.  The narrowing, the widening, the set-up and the replay are
mg_restatement's: a Problem is what its setup / replay / numpy_mgcg take in place of a list of levels."""
import math

import numpy as np

import mg_cases as mgc
import mg_restatement as rst
import mgcg_cases as mg

D, S = np.float64, np.float32


class Problem:
    """an outer f64 operator (a callable u -> A(u) on f64 arrays) and f32 levels whose level 0 has the outer
    operator's box and Omega"""

    def __init__(self, outer_A, levels):
        assert all(L.dt is S for L in levels) and len(levels) >= 2
        self.A, self.levels = outer_A, levels
        self.shape, self.where = levels[0].shape, levels[0].where


def star_problem(omega, n_levels, damp, texts64=None, texts32=None):
    """the unscaled Poisson star: outer operator lowered at f64, the levels' at f32; level 0's minv +0 outside Omega;
    -> (Problem, level 0's f64 module text, the f32 module texts)"""
    levels, texts32 = mg.star_levels(omega, n_levels, S, damp, texts=texts32)
    text64 = texts64 or mgc.mg_module(levels[0].shape, D)
    return Problem(rst.Operator(text64), levels), text64, texts32


def aniso_problem(omega, n_levels, weights, damp):
    """mgcg_cases' anisotropic star -sum_d weights[d] u_dd, outer at f64 and levels at f32"""
    levels, texts32 = mg.aniso_levels(omega, n_levels, weights, damp, dtype=S)
    text64 = mg.aniso_module(levels[0].shape, weights, D)
    return Problem(rst.Operator(text64), levels), text64, texts32


def true_residual(P: Problem, x, b0) -> float:
    """sum over Omega of (b - A(x))^2 in f64 by the oracle, the terms summed exactly"""
    q = P.A(x)
    d = (b0[P.where] - q[P.where]).astype(D)
    return math.fsum(float(v) * float(v) for v in d.ravel())


# ---------------------------------------------------------------- the device side of a Problem (GPU tests)
class Device:
    """what a GPU test hands to multigrid.cg_solve_mixed: outer (an f64 Level), h (the f32 Hierarchy, h.x[0] = z32 and
    h.b[0] = r32), x, b and work = [r, p, q]"""


def _bounds(where):
    return [s.start for s in where], [s.stop for s in where]


def device_problem(nh, P: Problem, entry64, entries32, x0, b0, others64=(), others32=None, offset=0) -> Device:
    """P on the device.  Every work field (r, p, q, r32, z32, q_l, and x_l, b_l for l >= 1) holds NaN before the call.
    offset: the fields the flat kernels stream (x, b, r, p, q, r32, z32, level 0's minv and q) start that many ELEMENTS into
    larger allocations -- 8 bytes for an f64 field, 4 for an f32 one with offset = 1: not 16-byte aligned.  A restatement
    level with `stages` gets them as line stages."""
    import solver_trace_cases as stc
    F = nh.fields.DeviceField
    make = (lambda a: stc.offset_field(nh, a, offset)) if offset else F.from_numpy
    nan = lambda shape, dt: np.full(shape, np.nan, dt)
    dev = Device()
    dev.outer = nh.mg.Level(entry64, F.from_numpy(np.zeros(P.shape, D)), _bounds(P.where), others=list(others64))
    levels = []
    for l, R in enumerate(P.levels):
        lines = [nh.mg.LineStage(ax, F.from_numpy(lo), F.from_numpy(inv), F.from_numpy(up)) for ax, lo, inv, up in getattr(R, "stages", [])]
        minv = make(R.minv) if l == 0 else F.from_numpy(R.minv)
        levels.append(nh.mg.Level(entries32[l], F.from_numpy(np.zeros(R.shape, S)), _bounds(R.where),
                                  others=list(others32[l]) if others32 else [], minv=minv, rscale=R.rscale, lines=lines))
    h = nh.mg.Hierarchy(levels)
    h.q = [make(nan(f.shape, S)) if l == 0 else F.from_numpy(nan(f.shape, S)) for l, f in enumerate(h.q)]
    h.x = [make(nan(P.shape, S))] + [F.from_numpy(nan(f.shape, S)) for f in h.x[1:]]
    h.b = [make(nan(P.shape, S))] + [F.from_numpy(nan(f.shape, S)) for f in h.b[1:]]
    dev.h, dev.x, dev.b = h, make(x0), make(b0)
    dev.work = [make(nan(P.shape, D)) for _ in range(3)]
    return dev
