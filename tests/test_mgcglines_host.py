"""neptune_hip_mgcg_solve_lines, neptune_hip_mg_line_first and neptune_hip_mg_line_smooth_dot without a GPU: the
exports and signatures, every new refusal on host pointers (the argument checks run before the device is touched), the
apply-free stage of the restatement against the plain stage on zero fields, the line-smoothed preconditioner as a dense
matrix, and the convergence the README's claim rests on -- conditions on the restatement (tests/mg_restatement.py), not on
the code under test."""
import ctypes as C
import inspect

import numpy as np
import pytest

import mg_restatement as rst
import mglines_cases as lc
from helpers import bits_equal, mismatch_report
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    return _capi.load()


# ---------------------------------------------------------------- exports and signatures
def test_exports_and_signatures(lib):
    counts = {"neptune_hip_mgcg_solve_lines": 17, "neptune_hip_mg_line_first": 9, "neptune_hip_mg_line_smooth_dot": 11}
    header = _capi.HEADER_PATH.read_text()
    for name, n_args in counts.items():
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f"{name}(" in header
        assert len(_capi.SIGNATURES[name][1]) == n_args
        # the header's parameter list has as many parameters
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(");")].count(",") + 1 == n_args, name
    # the one argument more than neptune_hip_mgcg_solve is `lines`, in second place
    plain, lines = _capi.SIGNATURES["neptune_hip_mgcg_solve"][1], _capi.SIGNATURES["neptune_hip_mgcg_solve_lines"][1]
    assert lines[0] is plain[0] and lines[1] is C.POINTER(_capi.MgLines) and list(lines[2:]) == list(plain[1:])
    from neptune_hip import multigrid
    for name in ("line_first", "line_smooth_dot"):
        assert callable(getattr(multigrid, name))
    assert inspect.signature(multigrid.cg_solve).parameters["lines"].default is False


# ---------------------------------------------------------------- refusals on host pointers
SHAPES = [(9, 17, 33), (5, 9, 17), (3, 5, 9)]      # Omega 7 x 15 x 31 -> 3 x 7 x 15 -> 1 x 3 x 7


class HostProblem:
    """three levels with one stage each (two on level 0), three work fields and a trace, all host memory: nothing may ever be
    launched on it"""

    def __init__(self, dtype=np.float64):
        self.arrays = [[np.zeros(s, dtype) for _ in range(4)] for s in SHAPES]     # x, b, q, minv per level
        self.factors = [[[np.zeros(s, dtype) for _ in range(3)] for _ in range(2)] for s in SHAPES]   # [level][stage][lo, inv, up]
        self.work = [np.zeros(SHAPES[0], dtype) for _ in range(3)]                 # r, p, z
        self.trace = np.zeros(3 * 4 + 64, dtype)
        self.levels = (_capi.MgLevel * len(SHAPES))()
        self.lines = (_capi.MgLines * len(SHAPES))()
        for l, s in enumerate(SHAPES):
            L = self.levels[l]
            L.fn, L.body = None, _capi.BODY_LAP3D7_F64
            L.g = make_geom(([0] * 3, list(s)), ([1] * 3, [n - 1 for n in s]))
            L.x, L.b, L.q, L.minv = (a.ctypes.data for a in self.arrays[l])
            L.rscale = 4.0
            S = self.lines[l]
            S.n_stages = 2 if l == 0 else 1
            for st in range(S.n_stages):
                S.axis[st] = 2 - st
                S.lo[st], S.inv[st], S.up[st] = (a.ctypes.data for a in self.factors[l][st])
        self.work_ptrs = [a.ctypes.data for a in self.work]
        self.trace_ptr = None
        self.lines_arg = self.lines

    def solve(self, lib, n_levels=3, dtype=_capi.F64, sweeps=2, coarse=8, max_iters=4, check_every=1, no_work=False, plain=False):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        warr = None if no_work else (C.c_void_p * 3)(*self.work_ptrs)
        rest = (None, sweeps, coarse, warr, max_iters, check_every, 0.0, self.trace_ptr, None, None, C.byref(done), C.byref(rr0),
                C.byref(last))
        if plain:
            rc = lib.neptune_hip_mgcg_solve(self.levels, n_levels, dtype, *rest)
        else:
            rc = lib.neptune_hip_mgcg_solve_lines(self.levels, self.lines_arg, n_levels, dtype, *rest)
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc


def _refused(lib, change=None, **kw):
    h = HostProblem()
    if change:
        change(h)
    return h.solve(lib, **kw) == _capi.EINVAL


@pytest.mark.parametrize("how", ["plain", "null", "empty"])
def test_without_lines_the_argument_checks_are_mgcg_solves(lib, how):
    """neptune_hip_mgcg_solve, lines = NULL and n_stages = 0 everywhere refuse the same requests"""
    def prepare(h):
        if how == "null":
            h.lines_arg = None
        elif how == "empty":
            h.lines_arg = (_capi.MgLines * len(SHAPES))()
    kw = {"plain": how == "plain"}

    def refused(change=None, **more):
        def both(h):
            prepare(h)
            if change:
                change(h)
        return _refused(lib, both, **kw, **more)
    assert refused(n_levels=1) and refused(sweeps=0) and refused(no_work=True)
    assert refused(n_levels=0) and refused(n_levels=17) and refused(dtype=7) and refused(dtype=_capi.F32)
    assert refused(coarse=-1) and refused(check_every=0) and refused(max_iters=-1)
    n_bytes = int(np.prod(SHAPES[0])) * 8
    for i in range(3):
        def null_work(h, i=i):
            h.work_ptrs[i] = None
        assert refused(null_work), i

        def misaligned(h, i=i):
            h.work_ptrs[i] += 4
        assert refused(misaligned), i
        for o in range(i):
            def same(h, i=i, o=o):
                h.work_ptrs[i] = h.work_ptrs[o] + n_bytes - 8
            assert refused(same), (i, o)
        for level in (0, 1):
            for field in ("x", "b", "q", "minv"):
                def onto_work(h, i=i, level=level, field=field):
                    setattr(h.levels[level], field, h.work_ptrs[i] + 8)
                assert refused(onto_work), (i, level, field)

        def trace_in_work(h, i=i):
            h.trace_ptr = h.work_ptrs[i] + 16
        assert refused(trace_in_work), i
    # without stages every level needs its minv
    for field in ("x", "b", "q", "minv"):
        for level in (0, 1, 2):
            assert refused(lambda h: setattr(h.levels[level], field, None)), (field, level)
    for level in (0, 1):
        for field in ("x", "b", "q", "minv"):
            def trace_in_field(h, level=level, field=field):
                h.trace_ptr = getattr(h.levels[level], field) + 8
            assert refused(trace_in_field), (level, field)


def test_new_solve_refusals_on_host_pointers(lib):
    # those neptune_hip_mg_solve_lines adds for `lines`
    for level in (0, 1, 2):
        for bad in (-1, 4):
            assert _refused(lib, lambda h: setattr(h.lines[level], "n_stages", bad)), (level, bad)
        for bad in (-1, 3):
            def bad_axis(h, level=level, bad=bad):
                h.lines[level].axis[0] = bad
            assert _refused(lib, bad_axis), (level, bad)
        for which in ("lo", "inv", "up"):
            def null_factor(h, level=level, which=which):
                getattr(h.lines[level], which)[0] = None
            assert _refused(lib, null_factor), (level, which)

            def misaligned(h, level=level, which=which):
                getattr(h.lines[level], which)[0] += 4
            assert _refused(lib, misaligned), (level, which)
            for field in ("x", "b", "q"):
                for other in {max(level - 1, 0), level, min(level + 1, 2)}:
                    def onto_field(h, level=level, which=which, field=field, other=other):
                        getattr(h.lines[level], which)[0] = getattr(h.levels[other], field) + 8
                    assert _refused(lib, onto_field), (level, which, field, other)
            # this call's own: a factor field may meet none of r, p, z, nor the trace
            for i in range(3):
                def onto_work(h, level=level, which=which, i=i):
                    getattr(h.lines[level], which)[0] = h.work_ptrs[i] + 8
                assert _refused(lib, onto_work), (level, which, i)

            def onto_trace(h, level=level, which=which):
                h.trace_ptr = h.trace.ctypes.data
                getattr(h.lines[level], which)[0] = h.trace.ctypes.data + 8
            assert _refused(lib, onto_trace), (level, which)
    # level 0's second stage is checked like its first
    def second_stage(h):
        h.lines[0].up[1] = h.work_ptrs[2] + 8
    assert _refused(lib, second_stage)
    # a level without stages still needs its minv
    def no_minv_no_stages(h):
        h.lines[2].n_stages = 0
        h.levels[2].minv = None
    assert _refused(lib, no_minv_no_stages)
    # ... and those of neptune_hip_mgcg_solve, with stages present (minv may be null: the other reason refuses)
    def without_minv(h):
        for l in range(3):
            h.levels[l].minv = None
    for kw in ({"n_levels": 1}, {"sweeps": 0}, {"no_work": True}, {"check_every": 0}, {"max_iters": -1}, {"coarse": -1}, {"dtype": 7}):
        assert _refused(lib, without_minv, **kw), kw
    for i in range(3):
        def work_on_level1(h, i=i):
            without_minv(h)
            h.work_ptrs[i] = h.levels[1].b + 8
        assert _refused(lib, work_on_level1), i
    vals = [C.c_int64(7) for _ in range(4)]
    lib.neptune_hip_mgcg_counts(*[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0, 0, 0, 0] and lib.neptune_hip_mgcg_rz0() == 0.0


def test_line_kernel_refusals_on_host_pointers(lib):
    h = HostProblem()
    xf, bf, qf, _ = (a.ctypes.data for a in h.arrays[0])
    lo, inv, up = (a.ctypes.data for a in h.factors[0][0])
    dot = np.zeros(2)
    d = dot.ctypes.data
    gf = C.byref(h.levels[0].g)
    E, F64 = _capi.EINVAL, _capi.F64
    n_bytes = int(np.prod(SHAPES[0])) * 8
    empty = make_geom(([0] * 3, list(SHAPES[0])), ([1, 1, 1], [1, 16, 32]))

    first = lambda dtype, g, axis, b, lo_, inv_, up_, x: lib.neptune_hip_mg_line_first(dtype, g, axis, b, lo_, inv_, up_, x, None)
    assert first(7, gf, 0, bf, lo, inv, up, xf) == E and first(F64, None, 0, bf, lo, inv, up, xf) == E
    assert first(F64, C.byref(empty), 0, bf, lo, inv, up, xf) == E
    for axis in (-1, 3):
        assert first(F64, gf, axis, bf, lo, inv, up, xf) == E
    good = [bf, lo, inv, up, xf]
    for i in range(5):
        args = list(good)
        args[i] = None
        assert first(F64, gf, 2, *args) == E, i
    for i in range(4):                     # x overlapping b, lo, inv or up
        args = list(good)
        args[i] = xf + n_bytes - 8
        assert first(F64, gf, 2, *args) == E, i

    sdot = lambda dtype, g, axis, q, b, lo_, inv_, up_, x, out: lib.neptune_hip_mg_line_smooth_dot(dtype, g, axis, q, b, lo_, inv_, up_, x,
                                                                                                   out, None)
    assert sdot(7, gf, 0, qf, bf, lo, inv, up, xf, d) == E and sdot(F64, None, 0, qf, bf, lo, inv, up, xf, d) == E
    assert sdot(F64, C.byref(empty), 0, qf, bf, lo, inv, up, xf, d) == E
    for axis in (-1, 3):
        assert sdot(F64, gf, axis, qf, bf, lo, inv, up, xf, d) == E
    good = [qf, bf, lo, inv, up, xf]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert sdot(F64, gf, 2, *args, d) == E, i
    for i in range(5):                     # x overlapping q, b, lo, inv or up
        args = list(good)
        args[i] = xf + n_bytes - 8
        assert sdot(F64, gf, 2, *args, d) == E, i
    for i in range(1, 5):                  # q overlapping b, lo, inv or up
        args = list(good)
        args[i] = qf + 8
        assert sdot(F64, gf, 2, *args, d) == E, i
    assert sdot(F64, gf, 2, *good, None) == E and sdot(F64, gf, 2, *good, d + 4) == E
    for f in good:
        assert sdot(F64, gf, 2, *good, f) == E and sdot(F64, gf, 2, *good, f + n_bytes - 8) == E
    assert not dot.any()


# ---------------------------------------------------------------- the apply-free stage of the restatement
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_first_stage_is_the_plain_stage_on_zero_fields(axis, dtype):
    """bit for bit, including lines whose right-hand side is -0 throughout: d = -0 - (+0) = -0 either way, and x = (+0) + e
    turns the resulting -0 into +0 in both"""
    shape, where = (7, 9, 12), (slice(1, 6), slice(2, 8), slice(1, 11))
    lower, diag, upper = lc.star_tridiagonal(shape, where, dtype)
    first, last = list(where), list(where)
    first[axis], last[axis] = where[axis].start, where[axis].stop - 1
    lower[tuple(first)] = 0.0
    upper[tuple(last)] = 0.0
    lo, inv, up = lc.factors(lower, diag, upper, where, axis, 0.8, outside=np.nan)
    rng = np.random.default_rng(5)
    b = rng.standard_normal(shape).astype(dtype)
    cut = [slice(None)] * 3
    cut[(axis + 1) % 3] = slice(3, 5)
    b[tuple(cut)] = -0.0
    junk = rng.standard_normal(shape).astype(dtype)
    zeros = np.zeros(shape, dtype)
    want = rst.line_stage(zeros, b, lo, inv, up, zeros, where, axis)
    got = rst.first_stage(b, lo, inv, up, zeros, where, axis)
    assert bits_equal(got, want), mismatch_report(got, want)
    assert (got[tuple(cut)] == 0).all() and not np.signbit(got[tuple(cut)]).any()      # whole lines of -0: +0 comes out
    assert np.count_nonzero(got[where]) > 0
    # x on Omega is not read, outside Omega it keeps its bits
    got = rst.first_stage(b, lo, inv, up, junk, where, axis)
    assert bits_equal(got[where], want[where])
    outside = np.ones(shape, bool)
    outside[where] = False
    assert bits_equal(got[outside], junk[outside])


# ---------------------------------------------------------------- the preconditioner as a dense matrix
@pytest.mark.parametrize("sweeps", [1, 2])
def test_the_line_smoothed_preconditioner_is_symmetric_positive_definite(sweeps, built_libs):
    """M with stages (0, 1) on every level of the flux hierarchy n = 17 (Omega 15 x 15 -> 7 x 7 -> 3 x 3 -> 1 x 1), omega = 0.8,
    8 coarse sweeps, column by column from unit vectors.  The bound on |M_ij - M_ji|: 16 S m eps ||M||_2 -- mgcg's bound of 16
    rounded operations per cell and stage application, S = the stage applications of one cycle (2 stages x 2 sweeps on three
    levels and 2 x 8 on the last: 28 for sweeps = 1, 40 for sweeps = 2), and m = 15, the line length: a tridiagonal solve
    carries a cell's rounding error along the whole line.
    Observed: max |M - M^T| = 8.9e-16 (sweeps = 1) and 4.4e-16 (sweeps = 2) against bounds of 1.1e-10 and 1.6e-10;
    ||M||_2 = 71.0 / 75.6; smallest eigenvalue 0.3292 / 0.3335."""
    levels, _, _ = lc.flux_levels((0, 1), n=17)
    assert [L.m for L in levels] == [(15, 15), (7, 7), (3, 3), (1, 1)]
    M = rst.dense_preconditioner(levels, sweeps=sweeps, coarse_sweeps=8)
    assert M.shape == (225, 225) and np.isfinite(M).all()
    norm = np.linalg.norm(M, 2)
    S = lc.stage_applications(levels, sweeps, 8)
    assert S == 12 * sweeps + 16
    bound = 16.0 * S * 15 * np.finfo(np.float64).eps * norm
    asym = float(np.abs(M - M.T).max())
    smallest = float(np.linalg.eigvalsh(0.5 * (M + M.T)).min())
    print(f"sweeps = {sweeps}: max |M - M^T| = {asym:.3e} (bound {bound:.3e}), ||M||_2 = {norm:.4f}, smallest eigenvalue {smallest:.4f}")
    assert asym <= bound
    assert smallest > 0.0


# ---------------------------------------------------------------- what the README's claim rests on
def _reached(seq, factor=1e-16):
    return next((k for k, v in enumerate(seq) if v <= factor * seq[0]), None)


def test_line_smoothed_cg_converges_where_the_point_preconditioner_crawls(built_libs):
    """Omega = 63 x 63, eps = 0.01, omega = 0.8, 8 coarse sweeps, b of mglines_cases.flux_problem, to rr <= 1e-16 rr_0.
    Pinned: stages (0, 1) arrive within 16 iterations with V(1, 1) and within 10 with V(2, 2); the point preconditioner V(2, 2)
    has not arrived after 20.
    Observed on the restatement: V(1, 1) with stages 8 iterations, V(2, 2) with stages 5; the point preconditioner has fallen
    to 1.2e-9 rr_0 after 20."""
    levels, _, _ = lc.flux_levels((0, 1))
    x0, b = lc.flux_problem(levels)
    assert levels[0].m == (63, 63)
    v11 = rst.numpy_mgcg(levels, x0, b, 16, sweeps=1, stop_at=0.0)
    v22 = rst.numpy_mgcg(levels, x0, b, 10, sweeps=2, stop_at=0.0)
    point_levels, _, _ = lc.flux_levels((), outside=0.0)
    point = rst.numpy_mgcg(point_levels, x0, b, 20, sweeps=2, stop_at=0.0)
    print(f"stages V(1,1): {_reached(v11)} iterations; V(2,2): {_reached(v22)}; point V(2,2): rr / rr_0 = {min(point) / point[0]:.3e} after 20")
    assert _reached(v11) is not None and _reached(v11) <= 16
    assert _reached(v22) is not None and _reached(v22) <= 10
    assert _reached(point) is None
