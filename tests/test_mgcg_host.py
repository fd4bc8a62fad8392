"""neptune_hip_mgcg_solve and neptune_hip_mg_smooth_dot without a GPU: the exports and signatures, every
refusal on host pointers (the argument checks run before the device is touched), the restatement's preconditioner as a dense
matrix, and the two conditions the GPU stop tests and the README's claim rest on -- conditions on the restatement
(tests/mgcg_cases.py), not on the code under test."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_restatement as rst
import mgcg_cases as mg
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    return _capi.load()


# ---------------------------------------------------------------- exports and signatures
def test_exports_and_signatures(lib):
    names = ["neptune_hip_mg_smooth_dot", "neptune_hip_mgcg_solve", "neptune_hip_mgcg_rz0", "neptune_hip_mgcg_counts"]
    header = _capi.HEADER_PATH.read_text()
    for name in names:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f"{name}(" in header
    assert len(_capi.SIGNATURES["neptune_hip_mgcg_solve"][1]) == 16
    assert len(_capi.SIGNATURES["neptune_hip_mg_smooth_dot"][1]) == 8
    vals = [C.c_int64(7) for _ in range(4)]
    lib.neptune_hip_mgcg_counts(*[C.byref(v) for v in vals])
    assert min(v.value for v in vals) >= 0
    lib.neptune_hip_mgcg_counts(None, None, None, None)
    assert lib.neptune_hip_mgcg_rz0() >= 0.0
    from neptune_hip import multigrid
    for name in ("cg_solve", "cg_counts", "cg_rz0", "smooth_dot"):
        assert callable(getattr(multigrid, name))


# ---------------------------------------------------------------- refusals on host pointers
SHAPES = [(9, 17, 33), (5, 9, 17), (3, 5, 9)]      # Omega 7 x 15 x 31 -> 3 x 7 x 15 -> 1 x 3 x 7


class HostProblem:
    """three levels, three work fields and a trace, all host memory: nothing may ever be launched on it"""

    def __init__(self, dtype=np.float64):
        self.arrays = [[np.zeros(s, dtype) for _ in range(4)] for s in SHAPES]     # x, b, q, minv per level
        self.work = [np.zeros(SHAPES[0], dtype) for _ in range(3)]                 # r, p, z
        self.trace = np.zeros(3 * 4 + 64, dtype)
        self.levels = (_capi.MgLevel * len(SHAPES))()
        for l, s in enumerate(SHAPES):
            L = self.levels[l]
            L.fn, L.body = None, _capi.BODY_LAP3D7_F64
            L.g = make_geom(([0] * 3, list(s)), ([1] * 3, [n - 1 for n in s]))
            L.x, L.b, L.q, L.minv = (a.ctypes.data for a in self.arrays[l])
            L.rscale = 4.0
        self.work_ptrs = [a.ctypes.data for a in self.work]
        self.trace_ptr = None

    def solve(self, lib, n_levels=3, dtype=_capi.F64, sweeps=2, coarse=8, max_iters=4, check_every=1, no_work=False):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        warr = None if no_work else (C.c_void_p * 3)(*self.work_ptrs)
        rc = lib.neptune_hip_mgcg_solve(self.levels, n_levels, dtype, None, sweeps, coarse, warr, max_iters, check_every, 0.0,
                                        self.trace_ptr, None, None, C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc


def _refused(lib, change=None, **kw):
    h = HostProblem()
    if change:
        change(h)
    return h.solve(lib, **kw) == _capi.EINVAL


def test_solve_refusals_on_host_pointers(lib):
    # its own
    assert _refused(lib, n_levels=1)                   # one level is pcg_solve
    assert _refused(lib, sweeps=0) and _refused(lib, sweeps=-1)
    assert _refused(lib, no_work=True)
    n_bytes = int(np.prod(SHAPES[0])) * 8
    for i in range(3):
        def null_work(h, i=i):
            h.work_ptrs[i] = None
        assert _refused(lib, null_work), i

        def misaligned(h, i=i):
            h.work_ptrs[i] += 4
        assert _refused(lib, misaligned), i
        for o in range(i):
            def same(h, i=i, o=o):
                h.work_ptrs[i] = h.work_ptrs[o] + n_bytes - 8          # starts in the other's last cell
            assert _refused(lib, same), (i, o)
        for level in (0, 1):
            for field in ("x", "b", "q", "minv"):
                def onto_work(h, i=i, level=level, field=field):
                    setattr(h.levels[level], field, h.work_ptrs[i] + 8)
                assert _refused(lib, onto_work), (i, level, field)

        def trace_in_work(h, i=i):
            h.trace_ptr = h.work_ptrs[i] + 16
        assert _refused(lib, trace_in_work), i
    for level in (0, 1):
        for field in ("x", "b", "q", "minv"):
            def trace_in_field(h, level=level, field=field):
                h.trace_ptr = getattr(h.levels[level], field) + 8
            assert _refused(lib, trace_in_field), (level, field)

    def trace_reaches_a_field(h):
        # the trace is 3 * max_iters = 12 values long: a work field that starts 10 values into it overlaps
        h.trace_ptr = h.trace.ctypes.data
        h.work_ptrs[1] = h.trace.ctypes.data + 10 * 8
    assert _refused(lib, trace_reaches_a_field)

    def trace_misaligned(h):
        h.trace_ptr = h.trace.ctypes.data + 4
    assert _refused(lib, trace_misaligned)
    # those of neptune_hip_mg_solve that apply
    assert _refused(lib, n_levels=0) and _refused(lib, n_levels=17) and _refused(lib, dtype=7)
    assert _refused(lib, dtype=_capi.F32)                   # the built-in body is an f64 one
    assert _refused(lib, coarse=-1) and _refused(lib, check_every=0) and _refused(lib, max_iters=-1)
    for field in ("x", "b", "q", "minv"):
        for level in (0, 1, 2):
            assert _refused(lib, lambda h: setattr(h.levels[level], field, None)), (field, level)

    def rank_differs(h):
        h.levels[1].g = make_geom(([0, 0], [9, 17]), ([1, 1], [8, 16]))
    assert _refused(lib, rank_differs)
    for d in range(3):
        def size_relation(h, d=d):
            ub = [n - 1 for n in SHAPES[1]]
            ub[d] -= 1
            h.levels[1].g = make_geom(([0] * 3, list(SHAPES[1])), ([1] * 3, ub))
        assert _refused(lib, size_relation), d

    def empty_omega(h):
        h.levels[0].g = make_geom(([0] * 3, list(SHAPES[0])), ([1, 1, 1], [1, 16, 32]))
    assert _refused(lib, empty_omega)

    def input0_box(h):
        s = SHAPES[0]
        h.levels[0].g = make_geom(([0] * 3, list(s)), ([1] * 3, [n - 1 for n in s]), [([1, 0, 0], [s[0] + 1, s[1], s[2]])])
    assert _refused(lib, input0_box)
    for a, b in (("x", "b"), ("x", "q"), ("x", "minv"), ("b", "q"), ("b", "minv"), ("q", "minv")):
        for level in (0, 1, 2):
            assert _refused(lib, lambda h: setattr(h.levels[level], a, getattr(h.levels[level], b) + 8)), (a, b, level)
    for a in ("x", "b", "q", "minv"):
        for b in ("x", "b", "q", "minv"):
            assert _refused(lib, lambda h: setattr(h.levels[1], a, getattr(h.levels[0], b) + 64)), (a, b)
            assert _refused(lib, lambda h: setattr(h.levels[2], a, getattr(h.levels[1], b) + 64)), (a, b)
    for bad in (float("nan"), float("inf")):
        assert _refused(lib, lambda h: setattr(h.levels[0], "rscale", bad))
        assert _refused(lib, lambda h: setattr(h.levels[1], "rscale", bad))

    def missing_fixed_input(h):
        s = SHAPES[0]
        box = ([0] * 3, list(s))
        h.levels[0].g = make_geom(box, ([1] * 3, [n - 1 for n in s]), [box, box])
    assert _refused(lib, missing_fixed_input)
    assert _refused(lib, lambda h: setattr(h.levels[0], "body", 99))
    assert lib.neptune_hip_mgcg_solve(None, 2, _capi.F64, None, 2, 8, None, 4, 1, 0.0, None, None, None, None, None, None) == _capi.EINVAL
    # a refused call reports no rz_0 and no iteration
    vals = [C.c_int64(7) for _ in range(4)]
    lib.neptune_hip_mgcg_counts(*[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0, 0, 0, 0] and lib.neptune_hip_mgcg_rz0() == 0.0


def test_smooth_dot_refusals_on_host_pointers(lib):
    h = HostProblem()
    xf, bf, qf, mf = (a.ctypes.data for a in h.arrays[0])
    dot = np.zeros(2)
    d = dot.ctypes.data
    gf = C.byref(h.levels[0].g)
    E = _capi.EINVAL
    call = lambda dtype, g, q, b, minv, x, out: lib.neptune_hip_mg_smooth_dot(dtype, g, q, b, minv, x, out, None)
    assert call(7, gf, qf, bf, mf, xf, d) == E
    assert call(_capi.F64, None, qf, bf, mf, xf, d) == E
    # the refusals of neptune_hip_mg_smooth
    for args in ((None, bf, mf, xf), (qf, None, mf, xf), (qf, bf, None, xf), (qf, bf, mf, None), (xf, bf, mf, xf), (qf, xf + 8, mf, xf),
                 (qf, bf, xf, xf)):
        assert call(_capi.F64, gf, *args, d) == E, args
    empty = make_geom(([0] * 3, list(SHAPES[0])), ([1, 1, 1], [1, 16, 32]))
    assert call(_capi.F64, C.byref(empty), qf, bf, mf, xf, d) == E
    # its own: a null, misaligned or overlapping dot_out
    assert call(_capi.F64, gf, qf, bf, mf, xf, None) == E
    assert call(_capi.F64, gf, qf, bf, mf, xf, d + 4) == E
    n_bytes = int(np.prod(SHAPES[0])) * 8
    for f in (qf, bf, mf, xf):
        assert call(_capi.F64, gf, qf, bf, mf, xf, f) == E
        assert call(_capi.F64, gf, qf, bf, mf, xf, f + n_bytes - 8) == E
    assert not dot.any()


# ---------------------------------------------------------------- the preconditioner as a dense matrix
@pytest.mark.parametrize("sweeps", [1, 2])
def test_the_preconditioner_is_symmetric_positive_definite(sweeps, built_libs):
    """M on Omega = 7 x 7, two levels, omega = 0.8, 8 coarse sweeps, column by column from unit vectors.
    The bound on |M_ij - M_ji|: a column passes S = 2 sweeps + 8 + 2 stages (sweeps, the two transfers, the coarse sweeps),
    each at most 16 rounded operations per cell (the five-point apply and the update: 10; the full-weighting stencil in two
    dimensions: 11; the interpolation: 4) of relative error eps / 2 each, and every stage after it is non-expansive up to the
    norm of M itself; so a column is off by at most 16 S (eps / 2) ||M||_2 and two entries differ by at most twice that:
    16 S eps ||M||_2.  Observed: 5.6e-17 (sweeps = 1) and 4.2e-17 (sweeps = 2) against bounds of 1.1e-13 and 1.3e-13;
    ||M||_2 = 2.66 / 2.73; smallest eigenvalue 0.092 / 0.119."""
    levels, _ = mg.star_levels((7, 7), 2, np.float64, 0.8)
    M = rst.dense_preconditioner(levels, sweeps=sweeps, coarse_sweeps=8)
    assert M.shape == (49, 49) and np.isfinite(M).all()
    norm = np.linalg.norm(M, 2)
    stages = 2 * sweeps + 8 + 2
    bound = 16.0 * stages * np.finfo(np.float64).eps * norm
    asym = float(np.abs(M - M.T).max())
    smallest = float(np.linalg.eigvalsh(0.5 * (M + M.T)).min())
    print(f"sweeps = {sweeps}: max |M - M^T| = {asym:.3e} (bound {bound:.3e}), ||M||_2 = {norm:.4f}, smallest eigenvalue {smallest:.4f}")
    assert asym <= bound
    assert smallest > 0.0


# ---------------------------------------------------------------- what the GPU stop tests and the README's claim rest on
CONVERGENCE = {
    # name: (Omega, levels, omega, dtype, iterations)
    "3d_f64": ((7, 15, 263), 3, 6.0 / 7.0, np.float64, 6),
    "2d_f64": ((15, 263), 3, 0.8, np.float64, 6),
    "3d_f32": ((7, 15, 263), 3, 6.0 / 7.0, np.float32, 3),
}


@pytest.mark.parametrize("name", sorted(CONVERGENCE))
def test_rr_falls_by_a_factor_of_four_per_iteration(name, built_libs):
    """tol_between's precondition on the problems of tests/test_mgcg_solve_gpu.py.  Observed factors per iteration: 3d_f64
    225, 202, 159, 184, 172, 147; 2d_f64 93, 95, 161, 55, 98, 95; 3d_f32 225, 202, 159."""
    omega, n_levels, damp, dtype, iters = CONVERGENCE[name]
    levels, _ = mg.star_levels(omega, n_levels, dtype, damp)
    x0, b = mgc.problem_fields(levels[0].shape, levels[0].where, dtype)
    seq = rst.numpy_mgcg(levels, x0, b, iters)
    print(name, [f"{a / c:.1f}" for a, c in zip(seq, seq[1:])])
    assert len(seq) == iters + 1
    for a, c in zip(seq, seq[1:]):
        assert c * 4.0 <= a, seq


ANISO_N = 39      # about 1.3 x the 30 iterations observed


def test_anisotropic_problem_preconditioned_cg_converges_where_cycles_stall(built_libs):
    """2-D, Omega = 63 x 63, operator -0.03 u_xx - u_yy unscaled, 5 levels, V(2, 2), omega = 0.8, 8 coarse sweeps, hashed b, to
    rr <= 1e-16 rr_0.  Observed on the restatement: the preconditioned iteration reaches it after 30 iterations; the plain
    cycles of mg_cases have fallen to 6.2e-10 rr_0 after 78 = 2 N cycles (they need 156).  Pinned: within N = 39 iterations,
    and not within 2 N cycles."""
    make = lambda: mg.aniso_levels((63, 63), 5, (0.03, 1.0), 0.8)[0]
    levels = make()
    L0 = levels[0]
    b = np.zeros(L0.shape)
    b[L0.where] = helpers.hash_field(L0.shape, np.float64, seed=91)[L0.where]
    x0 = np.zeros(L0.shape)
    seq = rst.numpy_mgcg(levels, x0, b, ANISO_N, stop_at=0.0)
    reached = next((k for k, v in enumerate(seq) if v <= 1e-16 * seq[0]), None)
    cycles = rst.rr_sequence(make(), x0, b, 2 * ANISO_N)
    print(f"preconditioned CG: {reached} iterations; V-cycles: rr / rr_0 = {cycles[-1] / cycles[0]:.3e} after {2 * ANISO_N} cycles")
    assert reached is not None and reached <= ANISO_N
    assert min(cycles) > 1e-16 * cycles[0]
