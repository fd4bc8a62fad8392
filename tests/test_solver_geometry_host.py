"""What tests/test_solver_geometry_gpu.py relies on, established without a device from the numpy recurrences on the oracle's
operator alone: the case generators emit today's text by default, bicg_cases.numpy_operator is the oracle's operator at every
rank and origin, and on every geometry of solver_geometry_cases the r . r sequences are finite and fall as the GPU tests
assume."""
import hashlib

import numpy as np
import pytest

import bicg_cases as bc
import cg_cases as cc
import helpers
import pcg_cases as pc
import solver_geometry_cases as gc
import solver_trace_cases as stc

# sha256 of the module texts the generators emitted for solver_trace_cases.PROBLEMS before they took origin and bounds:
# tests/golden/solver_traces.json pins bits produced from exactly these texts
DEFAULT_TEXT_SHA256 = {
    ("pcg", "f64_12x20x136"): "ab0e2bb35fb41f07d7072127a3410afdf5d52809eb5dee1f6ce24575d4bd2d78",
    ("bicg", "f64_12x20x136"): "c3b52e47836628e8d7f72915166f97c96c1978db564d72d32a273576cc121f79",
    ("pcg", "f32_12x20x136"): "b9cec132525c39fbbbb22d6079ffc7776d2347e69c02561278239167769d5ed8",
    ("bicg", "f32_12x20x136"): "901cef2bd846937f1d77b038e5f06c8fa73c61d31f3844fb119c0fccfc2143d8",
    ("pcg", "f64_9x11x131_rim"): "98a066616fdc76cffac9cc609f418643c0ad1d6eada0e659e1e481e58d44bf5b",
    ("bicg", "f64_9x11x131_rim"): "e5a948a16db5ea38ebc65313be881f3994c94a6f2b67b3a2e8292d11610f8556",
    ("pcg", "f32_9x11x131"): "0c1dbe106c4f6766a59fff0a1bdaa59e811d54c95556b1d9c5511dea1cb580f4",
    ("bicg", "f32_9x11x131"): "98772dbf8ffab430cc36a1e901449639ab4b87db716c0690a3227ccadc2c7ab4",
}


@pytest.mark.parametrize("name", list(stc.PROBLEMS))
def test_default_module_texts_are_the_ones_the_golden_traces_were_recorded_from(name):
    shape, dtype, rim = stc.PROBLEMS[name]
    sha = lambda text: hashlib.sha256(text.encode()).hexdigest()
    assert sha(pc.pcg_module(shape, dtype)) == DEFAULT_TEXT_SHA256[("pcg", name)]
    assert sha(bc.bicg_module(shape, dtype)) == DEFAULT_TEXT_SHA256[("bicg", name)]
    # ... and the Problem classes still build them, with the interior as bounds and Omega
    for P in (pc.Problem(shape, dtype, rim=rim), bc.Problem(shape, dtype, rim=rim)):
        assert sha(P.text) in DEFAULT_TEXT_SHA256.values()
        assert (list(P.bounds[0]), list(P.bounds[1])) == cc.interior(shape) and P.where == tuple(slice(1, n - 1) for n in shape)
    # the explicit form of the defaults is the same text
    assert pc.pcg_module(shape, dtype, [0, 0, 0], cc.interior(shape)) == pc.pcg_module(shape, dtype)
    assert bc.bicg_module(shape, dtype, [0, 0, 0], cc.interior(shape)) == bc.bicg_module(shape, dtype)


@pytest.mark.parametrize("name", ["r1_f64_1031_origin", "r1_f64_783_origin", "r1_f32_523", "r2_f64_37x261_origin", "r2_f32_19x131",
                                  "r3_f64_9x11x131_asym", "r3_f64_zero_trip"])
def test_numpy_operator_is_the_oracles_at_every_rank_and_origin(name):
    case = gc.CASES[name]
    rank = len(case.shape)
    A = bc.Operator(bc.bicg_module(case.shape, case.dtype, case.origin, case.bounds))
    u = helpers.hash_field(case.shape, case.dtype, seed=5)
    got, want = A(u), bc.numpy_operator(u, case.origin, case.bounds)
    assert helpers.bits_equal(got, want), helpers.mismatch_report(got, want)
    if case.empty:
        assert helpers.bits_equal(got, u)           # zero trips: the copy-through alone
        return
    # the coefficients, from a unit vector in the middle of Omega: centre 2 rank + sum c + sigma, lower neighbours 1 + c_d, upper 1
    where = gc.SOLVERS["bicgstab"].problem(case).where
    mid = tuple((s.start + s.stop) // 2 for s in where)
    e = np.zeros(case.shape, case.dtype)
    e[mid] = 1
    col = A(e)
    assert col[mid] == bc.centre_weight(rank) == 2 * rank + sum(bc.C_ADV[:rank]) + bc.SIGMA
    for d in range(rank):
        up, down = list(mid), list(mid)
        up[d] += 1
        down[d] -= 1
        assert col[tuple(up)] == -(1 + bc.C_ADV[d]) and col[tuple(down)] == -1
    assert np.count_nonzero(col) == 2 * rank + 1


def _preconditions(solver, P, A, where, minv, iters, tiny):
    S = gc.SOLVERS[solver]
    seq = S.numpy(P, A, where, minv, iters)
    print(solver, "rr:", [f"{v:.3e}" for v in seq])
    assert len(seq) == iters + 1 and all(np.isfinite(seq))
    if tiny:
        return seq
    at = min(iters, 6)
    assert seq[at] < 1e-2 * seq[0]
    if solver == "bicgstab":       # not monotone in general: over the iterations used it is
        assert all(seq[k + 1] < seq[k] for k in range(at))
    return seq


@pytest.mark.parametrize("name,solver", gc.pairs())
def test_every_geometry_case_is_a_solve_the_numpy_recurrences_converge_on(name, solver):
    case, P = gc.CASES[name], gc.problem(solver, name)
    lo = [b - o for b, o in zip(case.bounds[0], case.origin)]
    hi = [b - o for b, o in zip(case.bounds[1], case.origin)]
    assert P.where == tuple(slice(l, max(h, l)) for l, h in zip(lo, hi))         # Omega, physical, as the table states it
    iters = gc.iters_of(solver, name)
    seq = _preconditions(solver, P, P.A, P.where, P.minv, iters, case.tiny)
    if case.empty:
        assert seq == [0.0] * (iters + 1)
    if name == "r1_f32_3":
        # one unknown: alpha = rr / (4 rr) = 1 / 4 exactly (1 / 4 scaled by minv for PCG), so the residual is +0 after one
        # iteration and the second one runs on rr = 0
        assert seq[0] > 0 and seq[1:] == [0.0, 0.0]


@pytest.mark.parametrize("solver", list(gc.SOLVERS))
@pytest.mark.parametrize("name", list(gc.REGIONS))
def test_every_launch_region_leaves_a_solve_or_nothing(name, solver):
    case_name, region, empty = gc.REGIONS[name]
    case, P = gc.CASES[case_name], gc.problem(solver, case_name)
    A, where, minv = gc.restricted(P, region)
    assert empty == any(s.stop <= s.start for s in where)
    iters = gc.iters_of(solver, name)
    seq = _preconditions(solver, P, A, where, minv, iters, empty)
    if empty:
        assert seq == [0.0] * (iters + 1)
    # the graph test runs 10 iterations under this region and without one: finite throughout (its convergence claim is the one
    # established above, at the iterations established above)
    if name == gc.GRAPH_REGION:
        for AA, ww, mm in ((A, where, minv), (P.A, P.where, P.minv)):
            assert all(np.isfinite(gc.SOLVERS[solver].numpy(P, AA, ww, mm, 10)))


@pytest.mark.parametrize("name", list(gc.BUILTIN))
def test_builtin_bodies_give_finite_falling_sequences(name):
    """the built-in bodies are no model problems: no claim but that CG's and BiCGStab's r . r stay finite and fall over the
    iterations the GPU test runs"""
    P = gc.builtin_problem(name)
    for solver in ("cg", "bicgstab"):
        seq = gc.SOLVERS[solver].numpy(P, P.A, P.where, None, gc.BUILTIN_ITERS)
        print(name, solver, [f"{v:.3e}" for v in seq])
        assert all(np.isfinite(seq)) and all(v > 0 for v in seq) and seq[-1] < seq[0]
