"""Device-resident BiCGStab without a GPU: the library's new entry and its refusals, the Python signature, and
the test problem itself -- tests/bicg_cases.py's upwind advection-diffusion operator with the oracle's operator: it is the
operator the definition states, it is not symmetric, BiCGStab's recurrences converge on it where CG's do not, the recurrence's
r . r is the true residual's at the stop, and the stop tests have iterations to place their thresholds at."""
import ctypes as C
import inspect

import numpy as np
import pytest

import bicg_cases as bc
import cg_cases as cc
import helpers

SHAPES = {"f64_12x20x136": ((12, 20, 136), np.float64), "f64_9x11x131": ((9, 11, 131), np.float64),
          "f32_12x20x136": ((12, 20, 136), np.float32)}
_cache = {}


def _problem(name):
    if name not in _cache:
        shape, dtype = SHAPES[name]
        P = bc.Problem(shape, dtype)
        P.seq, P.x, P.r, P.p, P.rr0, P.trace = bc.numpy_bicgstab(P.A, P.x0, P.b, P.where, 24, full=True)
        _cache[name] = P
    return _cache[name]


def test_library_exports_the_bicgstab_solver(built_libs):
    from neptune_hip import _capi
    lib = _capi.load()          # raises AttributeError when a symbol of _capi.SIGNATURES is missing
    assert "neptune_hip_bicgstab_solve" in _capi.SIGNATURES
    restype, argtypes = _capi.SIGNATURES["neptune_hip_bicgstab_solve"]
    assert restype is C.c_int and len(argtypes) == 18
    assert argtypes == _capi.SIGNATURES["neptune_hip_cg_solve"][1]      # cg_solve's arguments; work holds five fields
    assert lib.neptune_hip_bicgstab_solve.restype is C.c_int


def test_python_entry_exists_with_the_stated_signature(built_libs):
    from neptune_hip import apply
    params = inspect.signature(apply.bicgstab_solve).parameters
    assert list(params)[:11] == ["entry", "x", "b", "bounds", "max_iters", "tol2", "check_every", "others", "trace", "dot", "cfg"]
    assert params["check_every"].default == 1 and params["others"].default == () and params["trace"].default is False
    assert params["dot"].default == "auto" and params["cfg"].default is None


def test_solver_refuses_bad_arguments_before_touching_a_device(built_libs):
    """the refusals of neptune_hip_bicgstab_solve run before the device is initialised: NEPTUNE_HIP_EINVAL on host buffers"""
    from neptune_hip import _capi
    from neptune_hip.geometry import make_geom
    lib = _capi.load()
    shape = (4, 5, 8)
    n = 4 * 5 * 8
    bufs = [(C.c_double * (n + 8))() for _ in range(7)]
    x, b, r, rh, p, v, t = [C.addressof(a) for a in bufs]
    box = ([0, 0, 0], list(shape))
    g = make_geom(box, ([1, 1, 1], [3, 4, 7]), [box], None)
    other = make_geom(box, ([1, 1, 1], [3, 4, 7]), [([0, 0, 0], [4, 5, 9])], None)     # input 0's box is not the result's
    done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)

    def solve(w=(r, rh, p, v, t), trace=None, max_iters=4, check_every=1, xp=x, bp=b, geom=g, body=_capi.BODY_LAP3D7_F64):
        return lib.neptune_hip_bicgstab_solve(None, None, body, _capi.F64, C.byref(geom), xp, bp, (C.c_void_p * 5)(*w),
                                              None, max_iters, check_every, 0.0, trace, None, None, C.byref(done), C.byref(rr0),
                                              C.byref(last))
    E = _capi.EINVAL
    assert solve(check_every=0) == E and solve(max_iters=-1) == E
    assert solve(xp=None) == E and solve(bp=None) == E
    assert solve(geom=other) == E and solve(body=-1) == E
    assert solve(xp=x + 4) == E                                           # misaligned for f64
    seven = [x, b, r, rh, p, v, t]
    for i in range(2, 7):                                                 # a null work field
        w = list(seven[2:])
        w[i - 2] = None
        assert solve(w=w) == E
    for i in range(7):                                                    # any two of the seven fields overlapping
        for j in range(i):
            for shift in (0, 8 * (n - 1)):                                # the same buffer; one cell shared
                f = list(seven)
                f[i] = seven[j] + shift
                assert solve(xp=f[0], bp=f[1], w=f[2:]) == E, (i, j, shift)
    spare = (C.c_double * (n + 40))()
    base = C.addressof(spare)
    for i in range(7):                                                    # a trace that overlaps a field
        assert solve(trace=seven[i] + 16) == E
        # the trace is 5 * max_iters = 20 values long: one that starts 19 values before a field reaches its first cell
        f = list(seven)
        f[i] = base + 19 * 8
        assert solve(xp=f[0], bp=f[1], w=f[2:], trace=base) == E
    assert solve(trace=base + 4) == E                                     # a misaligned trace
    assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_operator_is_the_one_the_definition_states(dtype):
    shape = (12, 20, 136)
    A = bc.Operator(bc.bicg_module(shape, dtype))
    u = helpers.hash_field(shape, dtype, seed=5)
    got, want = A(u), bc.numpy_operator(u)
    assert helpers.bits_equal(got, want), helpers.mismatch_report(got, want)
    # the coefficients, from unit vectors: centre 14, lower neighbours 5, 3, 2, upper neighbours 1 (with a minus sign)
    e = np.zeros(shape, dtype)
    e[5, 6, 7] = 1
    col = A(e)
    assert col[5, 6, 7] == 14 and (col[6, 6, 7], col[5, 7, 7], col[5, 6, 8]) == (-5, -3, -2)
    assert (col[4, 6, 7], col[5, 5, 7], col[5, 6, 6]) == (-1, -1, -1) and np.count_nonzero(col) == 7


def test_the_operator_is_not_symmetric():
    P = _problem("f64_12x20x136")
    u, w = np.zeros(P.shape), np.zeros(P.shape)
    u[P.where] = helpers.hash_field(P.shape, np.float64, seed=5)[P.where]      # zero rim: the operator the solver sees
    w[P.where] = helpers.hash_field(P.shape, np.float64, seed=6)[P.where]
    (uAw, bound_u), (wAu, bound_w) = cc.dot_terms(u, P.A(w), P.where), cc.dot_terms(w, P.A(u), P.where)
    print(f"u . A(w) = {uAw!r} (rounding bound {bound_u:.1e}), w . A(u) = {wAu!r} (rounding bound {bound_w:.1e})")
    # the two exact sums of rounded terms differ by a thousand times more than any rounding of the terms or of A could explain
    assert abs(uAw - wAu) > 1000.0 * (bound_u + bound_w)


@pytest.mark.parametrize("name,rel,cap", [("f64_12x20x136", 1e-8, 20), ("f64_9x11x131", 1e-8, 20), ("f32_12x20x136", 1e-6, 16)])
def test_bicgstab_converges_on_the_upwind_operator(name, rel, cap):
    P = _problem(name)
    seq = P.seq
    first = next((i for i, v in enumerate(seq) if v <= rel * seq[0]), None)
    print(name, "rr / rr_0:", [f"{v / seq[0]:.1e}" for v in seq], "first below", rel, ":", first)
    assert all(np.isfinite(seq)) and first is not None and first <= cap
    # the recomputed residual |b - A(x)|^2 agrees with the recurrence's rr within 1 % at the stop iteration
    rr0, trace = P.rr0, P.trace[:first]
    x, r, _, _ = bc.replay(P.A, P.x0, P.b, P.where, rr0, trace)
    true_r = P.b[P.where].astype(np.float64) - P.A(x)[P.where].astype(np.float64)
    rec = float(np.sum(r.astype(np.float64) ** 2))
    print("  true |b - A x|^2", float(np.sum(true_r ** 2)), "recurrence", rec, "sequence", seq[first])
    assert abs(float(np.sum(true_r ** 2)) - rec) <= 0.01 * rec
    assert abs(rec - seq[first]) <= 1e-3 * seq[first]


def test_cg_does_not_converge_on_the_upwind_operator():
    """what the solver is for: CG's recurrence r . r never gets below 1e-2 rr_0 in 40 iterations on this problem"""
    P = _problem("f64_12x20x136")
    seq = bc.numpy_cg_on(P.A, P.x0, P.b, P.where, 40)
    print("CG min rr / rr_0 over 40 iterations:", min(seq) / seq[0])
    assert min(seq) > 1e-2 * seq[0]


def test_bicgstab_converges_on_the_spd_operator_of_the_cg_tests():
    shape = (12, 20, 136)
    A = cc.Operator(cc.cg_module(shape, np.float64))
    where = tuple(slice(1, n - 1) for n in shape)
    b, x0 = helpers.hash_field(shape, np.float64, seed=71), np.zeros(shape, np.float64)
    seq = bc.numpy_bicgstab(A, x0, b, where, 10)
    print("rr / rr_0:", [f"{v / seq[0]:.1e}" for v in seq])
    assert all(np.isfinite(seq)) and min(seq) <= 1e-8 * seq[0]


@pytest.mark.parametrize("name,upto,least", [("f64_12x20x136", 12, 3), ("f64_9x11x131", 12, 3), ("f32_12x20x136", 8, 2)])
def test_the_stop_tests_have_iterations_to_place_thresholds_at(name, upto, least):
    """r . r is not monotone, so the GPU stop tests place their thresholds at bicg_cases.stop_points: at least three in the
    first 12 iterations for f64, two in the first 8 for f32"""
    P = _problem(name)
    pts = bc.stop_points(P.seq, upto)
    print(name, "stop points:", [(k, f"{t:.3e}") for k, t in pts])
    assert len(pts) >= least
    for k, tol2 in pts:
        # a factor sqrt(2) (to rounding) from the value that stops the loop and from every earlier one
        assert 1.4 * P.seq[k] <= tol2 and all(v >= 1.4 * tol2 for v in P.seq[:k])
        assert bc.expected_stop(P.seq, 1, 24, tol2) == (k, k)


@pytest.mark.parametrize("name", ["f64_12x20x136", "f32_12x20x136"])
def test_replay_and_numpy_bicgstab_are_one_definition(name):
    """replay() driven by numpy's own scalars walks numpy_bicgstab's path: the same x, r, p bit for bit, and each scalar within
    the bound of the replay's own terms"""
    P = _problem(name)
    iters = 4
    seq, x, r, p, rr0, trace = bc.numpy_bicgstab(P.A, P.x0, P.b, P.where, iters, full=True)
    xr, rr_, pr, checks = bc.replay(P.A, P.x0, P.b, P.where, rr0, trace)
    assert helpers.bits_equal(x, xr) and helpers.bits_equal(r, rr_) and helpers.bits_equal(p, pr)
    for k, row in enumerate(checks):
        for c, (ref, bound) in enumerate(row):
            assert abs(float(trace[k][c]) - ref) <= bound, (k, c)
    outside = np.ones(P.shape, bool)
    outside[P.where] = False
    zero = np.zeros(int(outside.sum()), P.dtype)
    assert helpers.bits_equal(r[outside], zero) and helpers.bits_equal(p[outside], zero)
