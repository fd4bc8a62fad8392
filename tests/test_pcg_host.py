"""Jacobi-preconditioned conjugate gradients without a GPU: the library's new entry, the Python signature, and
the test problem itself -- tests/pcg_cases.py's reaction-diffusion operator on 12x20x136 with the oracle's operator: the
preconditioner pays (a third of plain CG's iterations at most), r . r falls by at least 2x per iteration over the iterations
the GPU stop tests place their thresholds in, and the colour probing of apply.operator_diagonal returns the exact diagonal."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cg_cases as cc
import helpers
import pcg_cases as pc

SHAPE = (12, 20, 136)
_cache = {}


def _problem(dtype):
    if dtype not in _cache:
        _cache[dtype] = pc.Problem(SHAPE, dtype)
    return _cache[dtype]


def test_library_exports_the_preconditioned_solver(built_libs):
    from neptune_hip import _capi
    lib = _capi.load()          # raises AttributeError when a symbol of _capi.SIGNATURES is missing
    assert "neptune_hip_pcg_solve" in _capi.SIGNATURES and "neptune_hip_pcg_rz0" in _capi.SIGNATURES
    assert lib.neptune_hip_pcg_solve.restype is C.c_int and lib.neptune_hip_pcg_rz0.restype is C.c_double


def test_cg_solve_accepts_minv_and_the_helpers_exist(built_libs):
    from neptune_hip import apply
    sig = inspect.signature(apply.cg_solve)
    assert "minv" in sig.parameters and sig.parameters["minv"].default is None
    for fn in (apply.operator_diagonal, apply.jacobi_minv):
        params = inspect.signature(fn).parameters
        assert list(params)[:6] == ["entry", "like", "bounds", "others", "reach", "region"]
        assert params["reach"].default is None and params["region"].default is None


def test_preconditioned_solver_refuses_bad_arguments_before_touching_a_device(built_libs):
    """the refusals of neptune_hip_pcg_solve run before the device is initialised: NEPTUNE_HIP_EINVAL on host buffers"""
    from neptune_hip import _capi
    from neptune_hip.geometry import make_geom
    lib = _capi.load()
    shape = (4, 5, 8)
    n = 4 * 5 * 8
    bufs = [(C.c_double * (n + 8))() for _ in range(6)]
    x, b, r, p, q, m = [C.addressof(a) for a in bufs]
    box = ([0, 0, 0], list(shape))
    g = make_geom(box, ([1, 1, 1], [3, 4, 7]), [box], None)
    done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)

    def solve(minv=m, w=(r, p, q), trace=None, max_iters=4, check_every=1, xp=x):
        return lib.neptune_hip_pcg_solve(None, None, _capi.BODY_LAP3D7_F64, _capi.F64, C.byref(g), xp, b, minv, (C.c_void_p * 3)(*w),
                                         None, max_iters, check_every, 0.0, trace, None, None, C.byref(done), C.byref(rr0),
                                         C.byref(last))
    E = _capi.EINVAL
    assert solve(minv=None) == E                                         # a null minv
    assert solve(minv=m + 4) == E                                        # misaligned for f64
    for field in (x, b, r, p, q):
        assert solve(minv=field) == E and solve(minv=field + 8 * (n - 1)) == E    # minv overlaps a field
    assert solve(trace=m + 16) == E                                      # a trace inside minv
    # the trace is 3 * max_iters = 12 values long: one that starts 9 values before minv reaches into it (8 would not)
    both = (C.c_double * (n + 24))()
    assert solve(minv=C.addressof(both) + 16 * 8, trace=C.addressof(both) + 7 * 8) == E
    assert solve(check_every=0) == E and solve(max_iters=-1) == E and solve(xp=None) == E    # cg_solve's own refusals
    assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0) and lib.neptune_hip_pcg_rz0() == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_operator_is_the_one_the_issue_states(dtype):
    P = _problem(dtype)
    assert set(np.unique(P.w)) == set(dtype(v) for v in pc.W_VALUES)     # every value is drawn
    u = helpers.hash_field(SHAPE, dtype, seed=5)
    q = P.A(u)
    s = np.zeros_like(u[P.where])
    for ax in range(3):
        for sg in (-1, 1):
            sl = list(P.where)
            sl[ax] = slice(1 + sg, SHAPE[ax] - 1 + sg)
            s = (s + u[tuple(sl)]).astype(dtype)
    want = u.copy()
    want[P.where] = (((dtype(12) + P.w[P.where]) * u[P.where]).astype(dtype) - s).astype(dtype)
    assert helpers.bits_equal(q, want), helpers.mismatch_report(q, want)


def test_the_preconditioner_pays_on_the_test_problem():
    """numpy_pcg reaches rr <= 1e-8 rr_0 in at most a third of numpy_cg's iterations (f64)"""
    P = _problem(np.float64)
    ones = np.ones(SHAPE, np.float64)
    first = lambda seq: next(i for i, v in enumerate(seq) if v <= 1e-8 * seq[0])
    plain = pc.numpy_pcg(P.A, P.x0, P.b, ones, P.where, 40)
    # with minv = 1 the definition is plain CG's: the same sequence as cg_cases.numpy_cg on the same operator
    assert plain == cc.numpy_cg(P.A, P.x0, P.b, P.where, 40)
    pre = pc.numpy_pcg(P.A, P.x0, P.b, P.minv, P.where, 12)
    print(f"iterations to 1e-8: plain {first(plain)}, preconditioned {first(pre)}")
    assert 3 * first(pre) <= first(plain)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rr_falls_by_2x_per_iteration_where_the_stop_tests_look(dtype):
    P = _problem(dtype)
    iters = pc.STOP_ITERS[dtype]
    seq = pc.numpy_pcg(P.A, P.x0, P.b, P.minv, P.where, iters)
    ratios = [seq[i] / seq[i + 1] for i in range(iters)]
    print(np.dtype(dtype).name, "rr / rr_0:", [f"{v / seq[0]:.1e}" for v in seq], "min ratio", min(ratios))
    assert all(np.isfinite(seq)) and min(ratios) >= 2.0
    # before the rounding floor: the recurrence's r . r is still the true residual's, b - A(x) recomputed, within 1 %
    #   (checked at the last of these iterations; for f32 the true residual stalls near eps^2 * |b|^2 a few iterations later)
    x, r, _, _ = pc.replay(P.A, P.x0, P.b, P.minv, P.where, *_scalars(P, iters))
    true_r = (P.b[P.where].astype(np.float64) - P.A(x)[P.where].astype(np.float64))
    rec = float(np.sum(r.astype(np.float64) ** 2))
    print("  true |b - A x|^2", float(np.sum(true_r ** 2)), "recurrence", rec)
    assert abs(float(np.sum(true_r ** 2)) - rec) <= 0.01 * rec


def _scalars(P, iters):
    """(rz0, trace) as a device would report them, from a numpy run that sums with numpy: lets replay() run on the CPU"""
    dt = P.dtype
    r, p, _, _ = pc.setup(P.A, P.x0, P.b, P.minv, P.where)
    x = P.x0.copy()
    z = (P.minv * r).astype(dt)
    rz0 = rz = pc._sum((r * z).astype(dt))
    trace = []
    for _ in range(iters):
        q = P.A(p)
        pq = pc._sum((q[P.where] * p[P.where]).astype(dt))
        alpha = dt(rz / pq)
        x = (x + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * q).astype(dt)).astype(dt)
        z = (P.minv * r).astype(dt)
        rz_new = pc._sum((r * z).astype(dt))
        p = (z + (dt(rz_new / rz) * p).astype(dt)).astype(dt)
        trace.append((pq, rz_new, pc._sum((r * r).astype(dt))))
        rz = rz_new
    return rz0, trace


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_replay_and_numpy_pcg_are_one_definition(dtype):
    """replay() driven by numpy's own scalars walks numpy_pcg's path: its r . r terms sum to numpy_pcg's sequence"""
    P = _problem(dtype)
    iters = 4
    rz0, trace = _scalars(P, iters)
    seq = pc.numpy_pcg(P.A, P.x0, P.b, P.minv, P.where, iters)
    _, r, _, checks = pc.replay(P.A, P.x0, P.b, P.minv, P.where, rz0, trace)
    for k, (pq, rz, rr) in enumerate(checks):
        assert abs(float(trace[k][0]) - pq[0]) <= pq[1] and abs(float(trace[k][1]) - rz[0]) <= rz[1]
        assert abs(seq[k + 1] - rr[0]) <= rr[1] and float(trace[k][2]) == seq[k + 1]
    outside = np.ones(SHAPE, bool)
    outside[P.where] = False
    assert helpers.bits_equal(r[outside], np.zeros(int(outside.sum()), dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_probing_the_oracle_returns_the_exact_diagonal(dtype):
    P = _problem(dtype)
    got = pc.probe_diagonal(P.A, SHAPE, dtype, P.where, reach=1)
    assert helpers.bits_equal(got, P.diag), helpers.mismatch_report(got, P.diag)
    inside = got[P.where]
    assert helpers.bits_equal(inside, (dtype(12) + P.w[P.where]).astype(dtype)) and inside.min() == 12 and inside.max() == 4108
