"""Multigrid line smoothers without a GPU: the three new exports and the struct layout against the header, every
new refusal on host pointers (the argument checks run before the device is touched), the restatement of the line stage
(tests/mglines_cases.py) against dense solves, against the point sweep and on the cells the definition says are not read,
and the convergence preconditions the GPU stop test relies on -- conditions on the restatement, not on the code under test."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import mg_restatement as rst
import mglines_cases as lc
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    return _capi.load()


# ---------------------------------------------------------------- exports and layout
def test_exports_and_signatures(lib):
    header = " ".join(_capi.HEADER_PATH.read_text().split())
    for name in ("neptune_hip_mg_line_smooth", "neptune_hip_mg_solve_lines"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert ("int neptune_hip_mg_line_smooth(int dtype, const neptune_hip_apply_geom_t *g, int axis, void *q, const void *b, "
            "const void *lo, const void *inv, const void *up, void *x, void *stream);") in header
    assert ("int neptune_hip_mg_solve_lines(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, "
            "int n_levels, int dtype, int pre, int post, int coarse_sweeps, int64_t max_cycles, int64_t check_every, "
            "double tol2, double *rr_checks, void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *cycles_done, "
            "double *rr0, double *rr_last);") in header
    assert "typedef struct { int32_t n_stages; int32_t axis[3]; const void *lo[3], *inv[3], *up[3]; } neptune_hip_mg_lines_t;" in header
    assert len(_capi.SIGNATURES["neptune_hip_mg_line_smooth"][1]) == 10
    solve, lines = _capi.SIGNATURES["neptune_hip_mg_solve"][1], _capi.SIGNATURES["neptune_hip_mg_solve_lines"][1]
    assert len(lines) == 16 and lines[0] is solve[0] and lines[1] is C.POINTER(_capi.MgLines) and lines[2:] == solve[1:]


def test_lines_struct_layout_matches_the_header(lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "neptune_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(neptune_hip_mg_lines_t), offsetof(neptune_hip_mg_lines_t, n_stages),
         offsetof(neptune_hip_mg_lines_t, axis), offsetof(neptune_hip_mg_lines_t, lo), offsetof(neptune_hip_mg_lines_t, inv),
         offsetof(neptune_hip_mg_lines_t, up), sizeof(neptune_hip_mg_level_t));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", str(_capi.REPO_ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.MgLines
    assert got == [C.sizeof(S), S.n_stages.offset, S.axis.offset, S.lo.offset, S.inv.offset, S.up.offset, C.sizeof(_capi.MgLevel)]
    assert S.lo.offset == 16 and C.sizeof(S) == 88


# ---------------------------------------------------------------- refusals on host pointers
SHAPES = [(9, 17, 33), (5, 9, 17)]      # Omega 7 x 15 x 31 -> 3 x 7 x 15


class HostHierarchy:
    """two levels of host memory, each with x, b, q, minv and the factor fields of three stages: nothing may be launched"""

    def __init__(self, n_stages=(3, 1)):
        self.arrays = [[np.zeros(s) for _ in range(4)] for s in SHAPES]
        self.factors = [[[np.zeros(s) for _ in range(3)] for _ in range(3)] for s in SHAPES]      # [level][stage][lo, inv, up]
        self.levels = (_capi.MgLevel * 2)()
        self.lines = (_capi.MgLines * 2)()
        for l, s in enumerate(SHAPES):
            L = self.levels[l]
            L.fn, L.body = None, _capi.BODY_LAP3D7_F64
            L.g = make_geom(([0] * 3, list(s)), ([1] * 3, [n - 1 for n in s]))
            L.x, L.b, L.q, L.minv = (a.ctypes.data for a in self.arrays[l])
            L.rscale = 4.0
            S = self.lines[l]
            S.n_stages = n_stages[l]
            for st in range(3):
                S.axis[st] = st
                S.lo[st], S.inv[st], S.up[st] = (a.ctypes.data for a in self.factors[l][st])

    def solve(self, lib, lines=True):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mg_solve_lines(self.levels, self.lines if lines else None, 2, _capi.F64, 2, 2, 8, 4, 1, 0.0, None, None,
                                            None, C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc


def _refused(lib, change, **kw):
    h = HostHierarchy(**kw)
    change(h)
    return h.solve(lib) == _capi.EINVAL


def test_solve_lines_refusals_on_host_pointers(lib):
    for bad in (-1, 4, 7):
        assert _refused(lib, lambda h: setattr(h.lines[0], "n_stages", bad)), bad
        assert _refused(lib, lambda h: setattr(h.lines[1], "n_stages", bad)), bad
    for bad in (-1, 3):
        def axis(h, bad=bad):
            h.lines[0].axis[1] = bad
        assert _refused(lib, axis), bad
    for name in ("lo", "inv", "up"):
        for level, stage in ((0, 0), (0, 2), (1, 0)):
            def null(h):
                getattr(h.lines[level], name)[stage] = None
            assert _refused(lib, null), (name, level, stage)

            def misaligned(h):
                getattr(h.lines[level], name)[stage] = getattr(h.lines[level], name)[stage] + 4
            assert _refused(lib, misaligned), (name, level, stage)
            for field in ("x", "b", "q"):
                def own(h):
                    getattr(h.lines[level], name)[stage] = getattr(h.levels[level], field) + 8
                assert _refused(lib, own), (name, level, stage, field)

                def neighbour(h):
                    getattr(h.lines[level], name)[stage] = getattr(h.levels[1 - level], field) + 64
                assert _refused(lib, neighbour), (name, level, stage, field)
    # a level without stages needs its minv (that a level with stages may leave it out is shown on the device)
    assert _refused(lib, lambda h: setattr(h.levels[0], "minv", None), n_stages=(0, 1))
    assert _refused(lib, lambda h: setattr(h.levels[1], "minv", None), n_stages=(3, 0))
    # the refusals of neptune_hip_mg_solve still hold with lines, and with lines = NULL minv is required
    assert _refused(lib, lambda h: setattr(h.levels[0], "x", None))
    assert _refused(lib, lambda h: setattr(h.levels[1], "q", h.levels[1].b + 8))
    h = HostHierarchy()
    h.levels[0].minv = None
    assert h.solve(lib, lines=False) == _capi.EINVAL


def test_line_smooth_refusals_on_host_pointers(lib):
    h = HostHierarchy()
    x, b, q, _ = (a.ctypes.data for a in h.arrays[0])
    lo, inv, up = (a.ctypes.data for a in h.factors[0][0])
    g = C.byref(h.levels[0].g)
    E, f64 = _capi.EINVAL, _capi.F64
    call = lambda *a: lib.neptune_hip_mg_line_smooth(*a, None)
    assert call(7, g, 0, q, b, lo, inv, up, x) == E
    assert call(f64, None, 0, q, b, lo, inv, up, x) == E
    for axis in (-1, 3, 17):
        assert call(f64, g, axis, q, b, lo, inv, up, x) == E
    g2 = make_geom(([0, 0], [9, 17]), ([1, 1], [8, 16]))
    assert call(f64, C.byref(g2), 2, q, b, lo, inv, up, x) == E                      # axis 2 of a rank-2 field
    good = [q, b, lo, inv, up, x]
    for k in range(6):
        args = list(good)
        args[k] = None
        assert call(f64, g, 1, *args) == E, k
    for k in range(5):                                                              # x overlapping any other field
        args = list(good)
        args[k] = x + 8
        assert call(f64, g, 1, *args) == E, k
    for k in range(1, 5):                                                           # q overlapping any other field
        args = list(good)
        args[k] = q + 8
        assert call(f64, g, 1, *args) == E, k
    empty = make_geom(([0] * 3, list(SHAPES[0])), ([1, 1, 1], [1, 16, 32]))
    assert call(f64, C.byref(empty), 0, *good) == E


def test_python_layer_checks():
    from neptune_hip import multigrid

    class Like:
        def __init__(self, shape, dtype=_capi.F64):
            self.shape, self.rank, self.dtype = tuple(shape), len(shape), dtype
            self.lb, self.box = [0] * len(shape), ([0] * len(shape), list(shape))
    like = Like((9, 17))
    bounds = ([1, 1], [8, 16])
    f = Like((9, 17))
    stage = multigrid.LineStage(1, f, f, f)
    L = multigrid.Level(None, like, bounds, lines=[stage, (0, f, f, f)])
    assert [s.axis for s in L.lines] == [1, 0] and L.minv is None
    assert multigrid.Level(None, like, bounds).lines == []
    with pytest.raises(ValueError, match="three"):
        multigrid.Level(None, like, bounds, lines=[stage] * 4)
    with pytest.raises(ValueError, match="axis 2"):
        multigrid.Level(None, like, bounds, lines=[(2, f, f, f)])
    with pytest.raises(ValueError, match="box"):
        multigrid.Level(None, like, bounds, lines=[(0, f, Like((9, 18)), f)])
    with pytest.raises(ValueError, match="element type"):
        multigrid.Level(None, like, bounds, lines=[(0, f, f, Like((9, 17), _capi.F32))])


# ---------------------------------------------------------------- the restatement of the stage
def _random_tridiagonal(rng, shape, where, axis, dtype=np.float64):
    """a diagonally dominant T along `axis` on Omega (rim couplings +0), NaN outside Omega"""
    lower, diag, upper = (np.full(shape, np.nan, dtype) for _ in range(3))
    m = tuple(s.stop - s.start for s in where)
    lower[where] = rng.uniform(-1.0, 1.0, m)
    upper[where] = rng.uniform(-1.0, 1.0, m)
    diag[where] = rng.uniform(2.5, 4.0, m) * rng.choice([-1.0, 1.0], m)
    first, last = list(where), list(where)
    first[axis], last[axis] = where[axis].start, where[axis].stop - 1
    lower[tuple(first)] = 0.0
    upper[tuple(last)] = 0.0
    return lower, diag, upper


@pytest.mark.parametrize("m", [1, 2, 7])
@pytest.mark.parametrize("axis", [0, 1])
def test_stage_solves_the_tridiagonal_system(m, axis):
    """x_new - x = (T / omega)^-1 (b - q) per line, against np.linalg.solve on the dense matrix: 16 m eps relative"""
    rng = np.random.default_rng(100 * m + axis)
    omega = 0.8
    other = 5
    om = (m, other) if axis == 0 else (other, m)
    shape = (om[0] + 3, om[1] + 2)
    where = (slice(2, 2 + om[0]), slice(1, 1 + om[1]))
    lower, diag, upper = _random_tridiagonal(rng, shape, where, axis)
    lo, inv, up = lc.factors(lower, diag, upper, where, axis, omega)
    q, b, x = (rng.standard_normal(shape) for _ in range(3))
    got = rst.line_stage(q, b, lo, inv, up, x, where, axis)
    outside = np.ones(shape, bool)
    outside[where] = False
    assert np.array_equal(got[outside], x[outside])
    view = lambda f: np.moveaxis(f[where], axis, 0)
    e, d = view(got) - view(x), view(b) - view(q)
    worst = 0.0
    for line in range(other):
        T = np.diag(view(diag)[:, line]) + np.diag(view(lower)[1:, line], -1) + np.diag(view(upper)[:-1, line], 1)
        want = np.linalg.solve(T / omega, d[:, line])
        # e was recovered as (x + e) - x: allow that subtraction's rounding on top of the solve's bound
        bound = 16 * m * np.finfo(np.float64).eps * (np.abs(want).max() + np.abs(view(x)[:, line]).max())
        worst = max(worst, np.abs(e[:, line] - want).max() / bound)
        assert np.abs(e[:, line] - want).max() <= bound
    print(f"m = {m}, axis = {axis}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_cell_lines_are_the_point_sweep_bit_for_bit(dtype):
    rng = np.random.default_rng(3)
    shape, where = (4, 9), (slice(2, 3), slice(1, 8))            # m[0] = 1
    q, b, x, minv = (rng.standard_normal(shape).astype(dtype) for _ in range(4))
    nan = np.full(shape, np.nan, dtype)
    got = rst.line_stage(q, b, nan, minv, nan, x, where, 0)
    assert got.tobytes() == rst.smooth(q, b, minv, x, where).tobytes()
    # and the factors of a one-cell line are inv = 1 / (t / omega), lo = up = +0
    dt = np.dtype(dtype).type
    lower, diag, upper = _random_tridiagonal(rng, shape, where, 0, dtype)
    lo, inv, up = lc.factors(lower, diag, upper, where, 0, 0.8)
    assert np.array_equal(inv[where], (dt(1) / (diag[where] / dt(0.8)).astype(dt)).astype(dt))
    assert not lo.any() and not up.any() and not np.signbit(lo).any() and not np.signbit(up).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cells_that_are_not_read_leave_the_bits_alone(axis, dtype):
    rng = np.random.default_rng(11 + axis)
    shape, where = (6, 7, 9), (slice(1, 5), slice(2, 6), slice(1, 7))
    lower, diag, upper = (f.astype(dtype) for f in _random_tridiagonal(rng, shape, where, axis))
    lo, inv, up = lc.factors(lower, diag, upper, where, axis, 0.8)
    q, b, x = (rng.standard_normal(shape).astype(dtype) for _ in range(3))
    want = rst.line_stage(q, b, lo, inv, up, x, where, axis)
    outside = np.ones(shape, bool)
    outside[where] = False
    first, last = list(where), list(where)
    first[axis], last[axis] = where[axis].start, where[axis].stop - 1
    for poison in (np.nan, -0.0):
        lo2, inv2, up2, q2, b2 = (f.copy() for f in (lo, inv, up, q, b))
        for f in (lo2, inv2, up2, q2, b2):
            f[outside] = poison
        lo2[tuple(first)] = poison
        up2[tuple(last)] = poison
        got = rst.line_stage(q2, b2, lo2, inv2, up2, x, where, axis)
        assert got.tobytes() == want.tobytes(), poison
    assert np.isfinite(want).all()
    # the factor recurrence itself reads nothing outside Omega and no rim coupling
    l2, u2 = lower.copy(), upper.copy()
    l2[tuple(first)] = np.nan
    u2[tuple(last)] = np.nan
    again = lc.factors(l2, diag, u2, where, axis, 0.8)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(again, (lo, inv, up)))
    with pytest.raises(ValueError):
        bad = diag.copy()
        bad[tuple(s.start + 1 for s in where)] = 0.0 if axis else np.inf
        z = np.zeros(shape, dtype)
        lc.factors(z, bad, z, where, axis, 0.8)


def test_python_line_factors_are_the_restatements_bits():
    """multigrid.line_factors (what line_weights runs on the host) against the restatement, f64 and f32"""
    from neptune_hip import multigrid
    for dtype in (np.float64, np.float32):
        rng = np.random.default_rng(5)
        shape, where = (6, 7, 9), (slice(1, 5), slice(2, 6), slice(1, 7))
        for axis in range(3):
            T = [np.nan_to_num(f).astype(dtype) for f in _random_tridiagonal(rng, shape, where, axis)]
            got = multigrid.line_factors(*T, where, axis, 0.8)
            want = lc.factors(*T, where, axis, 0.8)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (dtype, axis)
    z = np.zeros((5, 5))
    with pytest.raises(ValueError):
        multigrid.line_factors(z, z, z, (slice(1, 4), slice(1, 4)), 0, 0.8)


def test_sweep_order_reverses_the_stages_after_the_coarse_correction():
    """pre-sweeps and coarse sweeps run stages 0 .. k-1, post-sweeps k-1 .. 0: recorded on a stub level"""
    calls = []

    class Stub(rst.Level):
        pass
    shape, where = (5, 5), (slice(1, 4), slice(1, 4))
    z = np.zeros(shape)
    L = Stub(lambda u: np.zeros_like(u), shape, where, z, np.float64)
    L.x, L.b, L.q = z.copy(), z.copy(), z.copy()
    one = np.ones(shape)
    L.stages = [(0, z, one, z), (1, z, one, z), (0, z, one, z)]
    real = rst.line_stage
    try:
        rst.line_stage = lambda q, b, lo, inv, up, x, where, axis: (calls.append(axis), real(q, b, lo, inv, up, x, where, axis))[1]
        rst.sweep(L)
        rst.sweep(L, reverse=True)
    finally:
        rst.line_stage = real
    L.stages = [(0, z, one, z), (1, z, one, z)]
    assert calls == [0, 1, 0, 0, 1, 0]
    calls.clear()
    try:
        rst.line_stage = lambda q, b, lo, inv, up, x, where, axis: (calls.append(axis), real(q, b, lo, inv, up, x, where, axis))[1]
        rst.sweep(L)
        rst.sweep(L, reverse=True)
    finally:
        rst.line_stage = real
    assert calls == [0, 1, 1, 0]


# ---------------------------------------------------------------- convergence preconditions of the GPU stop test
# The problem of DESIGN 3.17: the flux-form operator on 63 x 63, six levels 63 -> 1, V(2, 2), 8 coarse sweeps, omega = 0.8,
# b standard normal (flux_problem's seed), x0 = 0, restated with one rounding per operation in f64.  The observed figures
# are in the tests' docstrings; the tests print them again.
@pytest.fixture(scope="module")
def flux(built_libs):
    levels, _, _ = lc.flux_levels((0, 1))
    x0, b = lc.flux_problem(levels)
    return levels, x0, b


def test_flux_hierarchy(flux):
    levels, _, _ = flux
    assert [L.m for L in levels] == [(63, 63), (31, 31), (15, 15), (7, 7), (3, 3), (1, 1)]
    assert all(len(L.stages) == 2 and [s[0] for s in L.stages] == [0, 1] for L in levels)
    # the tridiagonal parts are those of the operator: A(u) = T_0 u + (the dim-1 couplings) on a random field
    L = levels[1]
    a, c = L.A.rest
    rng = np.random.default_rng(1)
    u = np.zeros(L.shape)
    u[L.where] = rng.standard_normal(L.m)
    lower0, diag, upper0 = lc.flux_tridiagonal(a, c, 0)
    lower1, _, upper1 = lc.flux_tridiagonal(a, c, 1)
    want = diag * u
    want[1:] += lower0[1:] * u[:-1]
    want[:-1] += upper0[:-1] * u[1:]
    want[:, 1:] += lower1[:, 1:] * u[:, :-1]
    want[:, :-1] += upper1[:, :-1] * u[:, 1:]
    assert np.allclose(L.A(u)[L.where], want[L.where], rtol=1e-13, atol=1e-13)


def test_alternating_lines_fall_by_a_factor_of_four_and_arrive(flux):
    """Observed: per-cycle factors of rr 9830.5, 219.5, 161.4, 150.2, 146.7, 145.0, 143.9 (worst of the first six 145.0);
    rr / rr0 = 6.2e-18 after 7 cycles (the unrounded float64 model on another right-hand side: 7 cycles, worst factor 136)."""
    levels, x0, b = flux
    seq = rst.rr_sequence(levels, x0, b, 14, stop_at=1e-16)
    factors = [a / c for a, c in zip(seq, seq[1:])]
    print("alternating:", [f"{f:.1f}" for f in factors], f"arrived after {len(seq) - 1} cycles, rr / rr0 = {seq[-1] / seq[0]:.2e}")
    assert len(seq) - 1 >= 6
    for f in factors[:6]:
        assert f >= 4.0, factors
    assert seq[-1] <= 1e-16 * seq[0] and len(seq) - 1 <= 14


@pytest.mark.parametrize("name,axes", [("point", ()), ("dim0", (0,)), ("dim1", (1,))])
def test_point_jacobi_and_single_directions_do_not_arrive(name, axes, built_libs):
    """Observed rr / rr0 after 28 cycles: point Jacobi 3.3e-05, lines along dim 0 only 3.4e-07, along dim 1 only 3.2e-05."""
    levels, _, _ = lc.flux_levels(axes)
    x0, b = lc.flux_problem(levels)
    seq = rst.rr_sequence(levels, x0, b, 28, stop_at=1e-16)
    print(f"{name}: rr / rr0 = {seq[-1] / seq[0]:.2e} after {len(seq) - 1} cycles")
    assert len(seq) - 1 == 28 and seq[-1] > 1e-16 * seq[0]
    assert math.isfinite(seq[-1])
