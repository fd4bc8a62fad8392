"""neptune_hip_mgcg_solve_mixed and neptune_hip_mg_smooth_dot_wide without a GPU: the exports and signatures,
the refusals on host pointers (the argument checks run before the device is touched), and what the claim "an f32 cycle costs
f64 CG no iteration" rests on -- conditions on the restatement (tests/mg_restatement.py), not on the code under test."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_restatement as rst
import mgcg_cases as mg
import mgcgmixed_cases as mx
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    return _capi.load()


# ---------------------------------------------------------------- exports and signatures
def test_exports_and_signatures(lib):
    header = _capi.HEADER_PATH.read_text()
    for name in ("neptune_hip_mgcg_solve_mixed", "neptune_hip_mg_smooth_dot_wide"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f"{name}(" in header
    assert len(_capi.SIGNATURES["neptune_hip_mgcg_solve_mixed"][1]) == 19
    assert len(_capi.SIGNATURES["neptune_hip_mg_smooth_dot_wide"][1]) == 9
    from neptune_hip import multigrid
    for name in ("cg_solve_mixed", "smooth_dot_wide", "cg_solve", "cg_counts", "cg_rz0"):
        assert callable(getattr(multigrid, name))


# ---------------------------------------------------------------- refusals on host pointers
SHAPES = [(9, 17, 33), (5, 9, 17), (3, 5, 9)]      # Omega 7 x 15 x 31 -> 3 x 7 x 15 -> 1 x 3 x 7


def _geom(shape, ub_shift=(0, 0, 0)):
    return make_geom(([0] * 3, list(shape)), ([1] * 3, [n - 1 - s for n, s in zip(shape, ub_shift)]))


class HostProblem:
    """an f64 outer level, three f32 levels, r, p and a trace, all host memory: nothing may ever be launched on it"""

    def __init__(self):
        self.outer_arrays = [np.zeros(SHAPES[0], np.float64) for _ in range(3)]       # x, b, q
        self.arrays = [[np.zeros(s, np.float32) for _ in range(4)] for s in SHAPES]   # x (z32), b (r32), q, minv per level
        self.factors = [np.zeros(SHAPES[1], np.float32) for _ in range(3)]            # a line stage on level 0 or 1
        self.work = [np.zeros(SHAPES[0], np.float64) for _ in range(2)]               # r, p
        self.trace = np.zeros(3 * 4 + 64, np.float64)
        self.outer = (_capi.MgLevel * 1)()
        O = self.outer[0]
        O.fn, O.body, O.g, O.rscale = None, _capi.BODY_LAP3D7_F64, _geom(SHAPES[0]), 4.0
        O.x, O.b, O.q = (a.ctypes.data for a in self.outer_arrays)
        self.levels = (_capi.MgLevel * len(SHAPES))()
        for l, s in enumerate(SHAPES):
            L = self.levels[l]
            L.fn, L.body, L.g, L.rscale = None, _capi.BODY_LAP3D27_F32, _geom(s), 4.0
            L.x, L.b, L.q, L.minv = (a.ctypes.data for a in self.arrays[l])
        self.lines = None
        self.work_ptrs = [a.ctypes.data for a in self.work]
        self.trace_ptr = None

    def line_stage_on(self, level):
        self.lines = (_capi.MgLines * len(SHAPES))()
        self.factors = [np.zeros(SHAPES[level], np.float32) for _ in range(3)]
        S = self.lines[level]
        S.n_stages = 1
        S.axis[0] = 2
        S.lo[0], S.inv[0], S.up[0] = (a.ctypes.data for a in self.factors)

    def solve(self, lib, n_levels=3, pair=(_capi.F64, _capi.F32), sweeps=2, coarse=8, max_iters=4, check_every=1, no_work=False,
              no_outer=False):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        warr = None if no_work else (C.c_void_p * 2)(*self.work_ptrs)
        rc = lib.neptune_hip_mgcg_solve_mixed(None if no_outer else self.outer, pair[0], None, self.levels, self.lines, n_levels, pair[1],
                                              sweeps, coarse, warr, max_iters, check_every, 0.0, self.trace_ptr, None, None,
                                              C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc


def _rc(lib, change=None, **kw):
    h = HostProblem()
    if change:
        change(h)
    return h.solve(lib, **kw)


def _refused(lib, change=None, **kw):
    return _rc(lib, change, **kw) == _capi.EINVAL


def test_a_wrong_dtype_pair_is_refused(lib):
    for pair in ((_capi.F64, _capi.F64), (_capi.F32, _capi.F32), (_capi.F32, _capi.F64), (7, _capi.F32), (_capi.F64, 7)):
        assert _refused(lib, pair=pair), pair


def test_counts_and_sizes_are_refused(lib):
    assert _refused(lib, n_levels=1) and _refused(lib, n_levels=0) and _refused(lib, n_levels=17)
    assert _refused(lib, sweeps=0) and _refused(lib, sweeps=-1) and _refused(lib, coarse=-1)
    assert _refused(lib, check_every=0) and _refused(lib, max_iters=-1)
    assert _refused(lib, no_work=True) and _refused(lib, no_outer=True)
    for field in ("x", "b", "q"):
        assert _refused(lib, lambda h: setattr(h.outer[0], field, None)), field
        assert _refused(lib, lambda h: setattr(h.outer[0], field, getattr(h.outer[0], field) + 4)), field
    for field in ("x", "b", "q", "minv"):
        for level in (0, 1, 2):
            assert _refused(lib, lambda h: setattr(h.levels[level], field, None)), (field, level)
    assert _refused(lib, lambda h: setattr(h.outer[0], "body", _capi.BODY_LAP3D27_F32))     # an f32 body for the f64 operator
    assert _refused(lib, lambda h: setattr(h.levels[0], "body", _capi.BODY_LAP3D7_F64))     # an f64 body in the f32 hierarchy
    assert _refused(lib, lambda h: setattr(h.outer[0], "body", 99))


def test_outer_and_level_zero_must_agree_in_box_and_omega(lib):
    for d in range(3):
        shift = [0, 0, 0]
        shift[d] = 1

        def one_cell_less(h, shift=tuple(shift)):
            h.outer[0].g = _geom(SHAPES[0], shift)          # Omega one cell shorter along d; the box is the same
        assert _refused(lib, one_cell_less), d

        def region_one_cell_less(h, d=d):
            h.outer[0].g.region_ub[d] = SHAPES[0][d] - 2      # the launch region ends one cell before the bounds do
        assert _refused(lib, region_one_cell_less), d

        def other_box(h, d=d):
            s = list(SHAPES[0])
            s[d] += 1
            g = make_geom(([0] * 3, s), ([1] * 3, [n - 1 for n in SHAPES[0]]))      # the same Omega in a larger box
            h.outer[0].g = g
        assert _refused(lib, other_box), d

    def other_rank(h):
        h.outer[0].g = make_geom(([0, 0], [17, 33]), ([1, 1], [16, 32]))
    assert _refused(lib, other_rank)


def test_overlaps_are_refused(lib):
    wide = int(np.prod(SHAPES[0])) * 8
    outer_fields = ("x", "b", "q")
    for i in range(2):
        def null_work(h, i=i):
            h.work_ptrs[i] = None
        assert _refused(lib, null_work), i

        def misaligned(h, i=i):
            h.work_ptrs[i] += 4
        assert _refused(lib, misaligned), i
        for field in outer_fields:
            def onto_outer(h, i=i, field=field):
                h.work_ptrs[i] = getattr(h.outer[0], field) + wide - 8      # starts in the field's last cell
            assert _refused(lib, onto_outer), (i, field)
        for level in (0, 1):
            for field in ("x", "b", "q", "minv"):
                def inner_onto_work(h, i=i, level=level, field=field):
                    setattr(h.levels[level], field, h.work_ptrs[i] + 8)
                assert _refused(lib, inner_onto_work), (i, level, field)

        def trace_in_work(h, i=i):
            h.trace_ptr = h.work_ptrs[i] + 16
        assert _refused(lib, trace_in_work), i

    def r_is_p(h):
        h.work_ptrs[1] = h.work_ptrs[0] + wide - 8
    assert _refused(lib, r_is_p)
    for a, b in (("x", "b"), ("x", "q"), ("b", "q")):
        assert _refused(lib, lambda h: setattr(h.outer[0], a, getattr(h.outer[0], b) + 8)), (a, b)
    for field in outer_fields:
        def trace_in_outer(h, field=field):
            h.trace_ptr = getattr(h.outer[0], field) + 8
        assert _refused(lib, trace_in_outer), field
        for level in (0, 1):
            for inner in ("x", "b", "q", "minv"):
                def inner_onto_outer(h, field=field, level=level, inner=inner):
                    setattr(h.levels[level], inner, getattr(h.outer[0], field) + 8)
                assert _refused(lib, inner_onto_outer), (field, level, inner)
    for level in (0, 1):
        for inner in ("x", "b", "q", "minv"):
            def trace_in_inner(h, level=level, inner=inner):
                h.trace_ptr = getattr(h.levels[level], inner) + 8
            assert _refused(lib, trace_in_inner), (level, inner)

    def trace_reaches_a_field(h):
        # the trace is 3 * max_iters = 12 doubles long: a work field that starts 10 values into it overlaps
        h.trace_ptr = h.trace.ctypes.data
        h.work_ptrs[1] = h.trace.ctypes.data + 10 * 8
    assert _refused(lib, trace_reaches_a_field)

    def trace_misaligned(h):
        h.trace_ptr = h.trace.ctypes.data + 4
    assert _refused(lib, trace_misaligned)
    # those of the inner hierarchy itself
    for a, b in (("x", "b"), ("x", "q"), ("x", "minv"), ("b", "q"), ("b", "minv"), ("q", "minv")):
        for level in (0, 1, 2):
            assert _refused(lib, lambda h: setattr(h.levels[level], a, getattr(h.levels[level], b) + 8)), (a, b, level)

    def factor_in_r(h):
        h.line_stage_on(1)
        h.lines[1].inv[0] = h.work_ptrs[0] + 8
    assert _refused(lib, factor_in_r)
    # a refused call reports no rz_0 and no iteration
    vals = [C.c_int64(7) for _ in range(4)]
    lib.neptune_hip_mgcg_counts(*[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0, 0, 0, 0] and lib.neptune_hip_mgcg_rz0() == 0.0


def test_a_line_stage_on_level_zero_is_unsupported(lib):
    assert _rc(lib, lambda h: h.line_stage_on(0)) == _capi.EUNSUPPORTED
    # ... also when level 0 then gives no minv, as neptune_hip_mgcg_solve_lines allows
    def without_minv(h):
        h.line_stage_on(0)
        h.levels[0].minv = None
    assert _rc(lib, without_minv) == _capi.EUNSUPPORTED


def test_smooth_dot_wide_refusals_on_host_pointers(lib):
    h = HostProblem()
    xf, bf, qf, mf = (a.ctypes.data for a in h.arrays[0])
    dot = np.zeros(2)
    d = dot.ctypes.data
    gf = C.byref(h.levels[0].g)
    E = _capi.EINVAL
    call = lambda pair, g, q, b, minv, x, out: lib.neptune_hip_mg_smooth_dot_wide(pair[0], pair[1], g, q, b, minv, x, out, None)
    ok = (_capi.F32, _capi.F64)
    for pair in ((_capi.F64, _capi.F64), (_capi.F32, _capi.F32), (_capi.F64, _capi.F32), (7, _capi.F64)):
        assert call(pair, gf, qf, bf, mf, xf, d) == E, pair
    assert call(ok, None, qf, bf, mf, xf, d) == E
    for args in ((None, bf, mf, xf), (qf, None, mf, xf), (qf, bf, None, xf), (qf, bf, mf, None), (xf, bf, mf, xf), (qf, xf + 8, mf, xf),
                 (qf, bf, xf, xf)):
        assert call(ok, gf, *args, d) == E, args
    assert call(ok, gf, qf, bf, mf, xf, None) == E
    assert call(ok, gf, qf, bf, mf, xf, d + 4) == E
    n_bytes = int(np.prod(SHAPES[0])) * 4
    for f in (qf, bf, mf, xf):
        assert call(ok, gf, qf, bf, mf, xf, f) == E
        assert call(ok, gf, qf, bf, mf, xf, f + n_bytes - 8) == E
    assert not dot.any()


# ---------------------------------------------------------------- the preconditioner in f32 as a dense matrix
def test_the_f32_preconditioner_is_symmetric_positive_definite(built_libs):
    """M32 on Omega = 7 x 7, two levels, omega = 0.8, V(2, 2), 8 coarse sweeps, column by column from unit vectors through
    the f32 levels.  The bound on |M_ij - M_ji| is the one of tests/test_mgcg_host.py with f32's eps: a column passes
    S = 2 sweeps + 8 + 2 stages of at most 16 rounded operations per cell, so two entries differ by at most
    16 S eps32 ||M||_2."""
    P, _, _ = mx.star_problem((7, 7), 2, 0.8)
    M = rst.dense_preconditioner(P.levels, sweeps=2, coarse_sweeps=8)
    assert M.shape == (49, 49) and np.isfinite(M).all()
    norm = np.linalg.norm(M, 2)
    bound = 16.0 * (2 * 2 + 8 + 2) * float(np.finfo(np.float32).eps) * norm
    asym = float(np.abs(M - M.T).max())
    smallest = float(np.linalg.eigvalsh(0.5 * (M + M.T)).min())
    print(f"max |M - M^T| = {asym:.3e} (bound {bound:.3e}), ||M||_2 = {norm:.4f}, smallest eigenvalue {smallest:.4f}")
    assert asym <= bound
    assert smallest > 0.0


# ---------------------------------------------------------------- an f32 cycle costs f64 CG no iteration
def _star(omega, n_levels, damp):
    P, _, _ = mx.star_problem(omega, n_levels, damp)
    return P, mg.star_levels(omega, n_levels, np.float64, damp)[0]


def _aniso(omega, n_levels, weights, damp):
    P, _, _ = mx.aniso_problem(omega, n_levels, weights, damp)
    return P, mg.aniso_levels(omega, n_levels, weights, damp)[0]


ITERATIONS = {
    # name: (how the mixed Problem and the all-f64 levels are built, the iterations both loops may run: about three times what
    # an independent experiment needed on problems of this kind -- 10 to 12 isotropic, 44 anisotropic; no bound of the test)
    "star_15x15x15": (lambda: _star((15, 15, 15), 3, 6.0 / 7.0), 40),
    "star_31x31": (lambda: _star((31, 31), 4, 0.8), 40),
    "aniso_31x31": (lambda: _aniso((31, 31), 4, (0.03, 1.0), 0.8), 120),
}


@pytest.mark.parametrize("name", sorted(ITERATIONS))
def test_to_1e_24_the_mixed_loop_needs_at_most_one_iteration_more_than_all_f64(name, built_libs):
    """V(2, 2), 8 coarse sweeps, hashed b, x0 = 0, to rr <= 1e-24 rr_0 -- far below anything f32 can express.  The mixed
    restatement may need at most one iteration more than mg_restatement.numpy_mgcg in f64 (an independent experiment found equal
    counts on five problems; the margin of one covers a different summation order), and the true residual b - A(x) of the
    mixed x, by the oracle in f64, must lie within a factor 4 of the recurrence's rr."""
    make, most = ITERATIONS[name]
    P, levels64 = make()
    b = np.zeros(P.shape)
    b[P.where] = helpers.hash_field(P.shape, np.float64, seed=91)[P.where]
    x0 = np.zeros(P.shape)
    rr0 = rst.numpy_mgcg(levels64, x0, b, 0)[0]
    stop = 1e-24 * rr0
    seq64 = rst.numpy_mgcg(levels64, x0, b, most, stop_at=stop)
    st, _, _, _, scalars = rst.replay(P, x0, b, iters=most, stop_at=stop)       # numpy_mgcg, and its x
    seq, x = [float(st.rr_own)] + [float(s[2]) for s in scalars], st.x
    true = mx.true_residual(P, x, b)
    print(f"{name}: all-f64 {len(seq64) - 1} iterations (rr / rr_0 = {seq64[-1] / rr0:.3e}), mixed {len(seq) - 1} iterations "
          f"(rr / rr_0 = {seq[-1] / rr0:.3e}); true residual of the mixed x {true:.6e} against the recurrence's {seq[-1]:.6e}")
    assert seq64[-1] <= stop and seq[-1] <= stop
    assert len(seq) - 1 <= len(seq64) - 1 + 1
    assert seq[-1] / 4.0 <= true <= seq[-1] * 4.0
