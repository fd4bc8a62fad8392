"""The geometries on which the three Krylov solvers are tested beyond rank 3, origin 0 and the whole interior (DESIGN 3.11 -
3.13), and ONE adapter per solver, so that one checker serves all three (tests/test_solver_geometry_gpu.py) and the CPU test of
the preconditions (tests/test_solver_geometry_host.py) runs the very same references.

A case is a box (shape, logical origin) and Omega given in PHYSICAL indices, [lo, hi) per dimension (None: one cell in from every
face); apply.bounds is Omega shifted by the origin.  A launch region is physical too.  With a region, Omega = bounds x region and
the operator stores nothing outside the region: the reference is the oracle's operator masked to +0 out there -- the reference
tests/test_bicg_solve_gpu.py uses.

Operators: cg_cases.cg_module (CG), pcg_cases.pcg_module with its coefficient field w and the Jacobi minv (PCG),
bicg_cases.bicg_module (BiCGStab).  b and x0 are hash fields (seeds 71 and 72): x0 is non-zero everywhere, so every cell outside
Omega is boundary data that must come back bit for bit."""
import numpy as np

import bicg_cases as bc
import cg_cases as cc
import helpers
import monitor_cases as mc
import pcg_cases as pc


class Case:
    def __init__(self, shape, dtype, origin=None, lo=None, hi=None, iters=None, tiny=False, solvers=("cg", "pcg", "bicgstab")):
        rank = len(shape)
        self.shape, self.dtype = tuple(shape), dtype
        self.origin = tuple([0] * rank if origin is None else origin)
        lo = [1] * rank if lo is None else lo
        hi = [n - 1 for n in shape] if hi is None else hi
        # apply.bounds, logical
        self.bounds = ([o + l for o, l in zip(self.origin, lo)], [o + h for o, h in zip(self.origin, hi)])
        self.iters = iters if iters is not None else (6 if dtype == np.float64 else 5)
        self.tiny = tiny                 # no convergence claim
        self.solvers = solvers
        self.empty = any(h <= l for l, h in zip(lo, hi))


CASES = {
    # rank 1, 5 row chunks, odd n.  Not BiCGStab: on the rank-1 upwind operator (centre 7, lower 5, upper 1) its r . r rises at the
    # third iteration for every odd n from 875 to 1099 (at n = 1031: 2.8e4, 1.1e3, 3.0e2, 5.6e2, 7.5e2, 1.3e1, 3.6e1), so the case
    # has another shape for it: 4 row chunks, odd n, falling steadily over 6 iterations (2.2e4 -> 5.0)
    "r1_f64_1031_origin": Case((1031,), np.float64, (7,), [2], [1026], solvers=("cg", "pcg")),
    "r1_f64_783_origin": Case((783,), np.float64, (7,), [2], [778], solvers=("bicgstab",)),
    "r1_f32_523": Case((523,), np.float32),                                            # rank 1, n % 4 == 3
    # fewer cells than one 16-byte group; one unknown: exact convergence, then an iteration with alpha = beta = 0
    "r1_f32_3": Case((3,), np.float32, None, [1], [2], iters=2, tiny=True),
    "r2_f64_37x261_origin": Case((37, 261), np.float64, (-3, 5), [2, 1], [36, 257]),   # rank 2, a row longer than 256
    "r2_f32_19x131": Case((19, 131), np.float32),                                      # rank 2, the f32 tail
    # three different lo, three different n - hi, a shifted origin
    "r3_f64_9x11x131_asym": Case((9, 11, 131), np.float64, (3, -2, 5), [1, 2, 3], [7, 10, 128]),
    "r3_f64_zero_trip": Case((9, 11, 131), np.float64, None, [4, 1, 1], [4, 10, 130], tiny=True),   # empty Omega
}
# BiCGStab's r . r is not monotone: where the numpy run does not fall steadily over the case's iterations, the case runs the
# iterations over which it does (tests/test_solver_geometry_host.py holds every entry to the same assertions)
ITERS_OF = {("bicgstab", "r2_f64_37x261_origin"): 2,      # 4.5e5, 1.2e4, 1.7e3, then 2.0e3
            ("bicgstab", "r3_dim0_cuts_omega"): 4,        # 3.2e5, 4.9e3, 4.6e2, 7.4e1, 1.5e1, then 3.5e1
            ("bicgstab", "r3_last_dim"): 4,               # 2.2e5, 3.9e3, 4.3e2, 9.2e1, 2.6e1, then 1.4e5
            ("bicgstab", "r2_dim1"): 2}                   # 2.3e5, 6.0e3, 8.6e2, then 1.9e3
ZERO_TRIP = "r3_f64_zero_trip"
ASYM = "r3_f64_9x11x131_asym"

# name: (case, launch region (physical), whether Omega = bounds x region is empty)
REGIONS = {
    "r3_dim0_cuts_omega": (ASYM, ([2, 0, 0], [6, 11, 131]), False),
    "r3_last_dim": (ASYM, ([0, 0, 40], [9, 11, 100]), False),
    "r2_dim1": ("r2_f64_37x261_origin", ([0, 130], [37, 261]), False),      # cuts Omega's lower end along dim 1, not its upper
    "r3_disjoint": (ASYM, ([7, 0, 0], [9, 11, 131]), True),                 # Omega's dim 0 is [1, 7)
}
GRAPH_REGION = "r3_dim0_cuts_omega"

# built-in bodies: name -> (the oracle's kind, shape); f64, origin 0, interior bounds
BUILTIN = {"BODY_LAP3D7_F64": ("3d7", (9, 11, 131)), "BODY_LAP2D5_F64": ("2d5", (19, 261))}
BUILTIN_ITERS = 4


class Problem:
    """one (solver, case), built once and left unchanged: the module text, the oracle's operator, b, x0, Omega (`where`,
    physical), and for PCG the coefficient field w"""


class _Solver:
    """What differs between the solvers, for one checker.  A, where, minv: the reference operator, Omega and (PCG) the
    preconditioner of THIS run -- the problem's own, or those of a launch region (restricted())."""
    minv_needed = False

    def problem(self, case: Case) -> Problem:
        P = Problem()
        P.shape, P.dtype, P.origin, P.bounds = case.shape, case.dtype, case.origin, case.bounds
        P.where = mc.inside_slices(P.shape, P.origin, P.bounds)
        P.b = helpers.hash_field(P.shape, P.dtype, seed=71)
        P.x0 = helpers.hash_field(P.shape, P.dtype, seed=72)
        P.w = P.minv = None
        self._operator(P)
        for a in (P.b, P.x0):
            a.setflags(write=False)
        return P


class _Cg(_Solver):
    name, work, scalars, rr_col = "cg", ("r", "p", "q"), ("pq", "rr'"), 1
    zero_outside = ("r", "p")

    def _operator(self, P):
        P.text = cc.cg_module(P.shape, P.dtype, P.origin, P.bounds)
        P.A = cc.Operator(P.text)

    def numpy(self, P, A, where, minv, iters):
        return cc.numpy_cg(A, P.x0, P.b, where, iters)

    def setup(self, P, A, where, minv):
        """-> (the vectors after the set-up, {name of a start scalar: (terms' sum, bound)})"""
        r, p, rr0 = cc.setup(A, P.x0, P.b, where)
        return {"r": r, "p": p}, {"rr0": rr0}

    def replay(self, P, A, where, minv, start, trace):
        """start: the DEVICE's start scalars by name.  -> (the vectors, checks[k][c] = (terms' sum, bound) of trace[k][c])"""
        x, r, p, checks = cc.replay(A, P.x0, P.b, where, start["rr0"], trace)
        return {"x": x, "r": r, "p": p}, checks

    def solve(self, nh, entry, x, b, bounds, work, minv, others, max_iters, tol2, **kw):
        return nh.apply.cg_solve(entry, x, b, bounds, max_iters, tol2, work=work, others=others, **kw)

    def start(self, nh, rr0):
        return {"rr0": rr0}


class _Pcg(_Cg):
    name, scalars, rr_col = "pcg", ("pq", "rz'", "rr'"), 2
    minv_needed = True

    def _operator(self, P):
        P.text = pc.pcg_module(P.shape, P.dtype, P.origin, P.bounds)
        P.w = pc.w_field(P.shape, P.dtype)
        P.w.setflags(write=False)
        P.A = pc.Operator(P.text, P.w)
        P.minv = numpy_minv(P.w, P.where)

    def numpy(self, P, A, where, minv, iters):
        return pc.numpy_pcg(A, P.x0, P.b, minv, where, iters)

    def setup(self, P, A, where, minv):
        r, p, rz0, rr0 = pc.setup(A, P.x0, P.b, minv, where)
        return {"r": r, "p": p}, {"rz0": rz0, "rr0": rr0}

    def replay(self, P, A, where, minv, start, trace):
        x, r, p, checks = pc.replay(A, P.x0, P.b, minv, where, start["rz0"], trace)
        return {"x": x, "r": r, "p": p}, checks

    def solve(self, nh, entry, x, b, bounds, work, minv, others, max_iters, tol2, **kw):
        return nh.apply.cg_solve(entry, x, b, bounds, max_iters, tol2, work=work, others=others, minv=minv, **kw)

    def start(self, nh, rr0):
        return {"rz0": nh.apply.pcg_rz0(), "rr0": rr0}


class _Bicgstab(_Solver):
    name, work, scalars, rr_col = "bicgstab", ("r", "rh", "p", "v", "t"), ("rv", "ts", "tt", "rho'", "rr'"), 4
    zero_outside = ("r", "rh", "p")

    def _operator(self, P):
        P.text = bc.bicg_module(P.shape, P.dtype, P.origin, P.bounds)
        P.A = bc.Operator(P.text)

    def numpy(self, P, A, where, minv, iters):
        return bc.numpy_bicgstab(A, P.x0, P.b, where, iters)

    def setup(self, P, A, where, minv):
        r, rh, p, rr0 = bc.setup(A, P.x0, P.b, where)
        return {"r": r, "rh": rh, "p": p}, {"rr0": rr0}

    def replay(self, P, A, where, minv, start, trace):
        x, r, p, checks = bc.replay(A, P.x0, P.b, where, start["rr0"], trace)
        return {"x": x, "r": r, "p": p, "rh": bc.setup(A, P.x0, P.b, where)[1]}, checks

    def solve(self, nh, entry, x, b, bounds, work, minv, others, max_iters, tol2, **kw):
        return nh.apply.bicgstab_solve(entry, x, b, bounds, max_iters, tol2, work=work, others=others, **kw)

    def start(self, nh, rr0):
        return {"rr0": rr0}


SOLVERS = {"cg": _Cg(), "pcg": _Pcg(), "bicgstab": _Bicgstab()}
_problems = {}


def pairs(names=None):
    """-> [(case, solver)] over the cases each solver runs"""
    return [(name, solver) for name in (CASES if names is None else names) for solver in SOLVERS if solver in CASES[name].solvers]


def iters_of(solver, name):
    """the iterations (solver, case or region) runs, and after which r . r is below 1e-2 rr_0 unless the case is tiny or empty"""
    case = CASES[REGIONS[name][0]] if name in REGIONS else CASES[name]
    return ITERS_OF.get((solver, name), case.iters)


def problem(solver: str, case: str) -> Problem:
    if (solver, case) not in _problems:
        _problems[(solver, case)] = SOLVERS[solver].problem(CASES[case])
    return _problems[(solver, case)]


def numpy_minv(w, where):
    """jacobi_minv's field from the exact diagonal: 1 / (4 rank + w) on Omega, 1 elsewhere"""
    m = pc.minv_of(pc.diagonal(w, where), where)
    m.setflags(write=False)
    return m


def restricted(P: Problem, region):
    """the reference of a run under a launch region: -> (A masked to +0 outside the region, Omega = bounds x region as physical
    slices, the Jacobi minv of that Omega or None); region None: the problem's own"""
    if region is None:
        return P.A, P.where, P.minv
    where = tuple(slice(max(w.start, lo), max(min(w.stop, hi), max(w.start, lo))) for w, lo, hi in zip(P.where, *region))
    inside = np.zeros(P.shape, bool)
    inside[tuple(slice(lo, hi) for lo, hi in zip(*region))] = True

    def A(u):
        return np.where(inside, P.A(u), P.dtype(0))
    return A, where, (None if P.w is None else numpy_minv(P.w, where))


def builtin_operator(kind):
    """the oracle's built-in body `kind` on its interior, as an operator"""
    return lambda u: helpers.oracle_entry(kind, u)


def builtin_problem(name) -> Problem:
    if name not in _problems:
        kind, shape = BUILTIN[name]
        P = Problem()
        P.shape, P.dtype, P.origin, P.bounds = shape, np.float64, (0,) * len(shape), cc.interior(shape)
        P.where = tuple(slice(1, n - 1) for n in shape)
        P.b = helpers.hash_field(shape, np.float64, seed=71)
        P.x0 = helpers.hash_field(shape, np.float64, seed=72)
        P.w = P.minv = None
        P.A = builtin_operator(kind)
        for a in (P.b, P.x0):
            a.setflags(write=False)
        _problems[name] = P
    return _problems[name]
