"""neptune_hip_cg_solve, _pcg_solve and _bicgstab_solve on the geometries their own modules never reach
(tests/solver_geometry_cases.py): rank 1 and 2, shifted origins, an Omega with different margins on every face, launch regions
under CG and PCG and along other dimensions than dim 0, built-in bodies, a set-up grid folded into two dimensions, a field
smaller than one 16-byte group, an empty Omega, and one cached graph followed by the same entry and fields under another region.

ONE checker for all three solvers, parametrised by the adapters of solver_geometry_cases.SOLVERS.  It asserts what the
_check_replay of test_cg_solve_gpu.py, test_pcg_solve_gpu.py and test_bicg_solve_gpu.py assert: the replay of the definition
driven by the device's own scalars reproduces every vector bit for bit, every scalar lies within the dot_terms bound
2 (n - 1) eps sum |t_i| of the exact sum of the replay's own terms, x is unchanged outside Omega, the residual vectors are +0
there, nothing of the NaN the work fields held is left, the counters add up, and r . r has fallen below 1e-2 rr_0 where
tests/test_solver_geometry_host.py established that from the numpy recurrences."""
import math

import numpy as np
import pytest

import helpers
import pcg_cases as pc
import solver_geometry_cases as gc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

DOTS = ("auto", "fallback")
CHECK_EVERY = 2


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    import os
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache"))
    from neptune_hip import _capi, apply, fields, lowering

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering = torch, _capi, apply, fields, lowering
    ns.lib = _capi.load()
    ns.lib.neptune_hip_init(0)
    ns.entries, ns.keep = {}, []
    # every case's module, compiled side by side
    helpers.prefetch_modules([lowering.with_options(gc.problem(solver, name).text, dot_entries=True) for name, solver in gc.pairs()])
    return ns


def _entry(nh, solver, name):
    if (solver, name) not in nh.entries:
        text = gc.problem(solver, name).text
        nh.entries[(solver, name)] = nh.lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    return nh.entries[(solver, name)]


class Run:
    """the device fields of one solve: x, b, the work fields, and for PCG w and minv"""


def _fields(nh, S, P, minv):
    F = nh.fields.DeviceField
    R = Run()
    R.x, R.b = F.from_numpy(P.x0, lb=P.origin), F.from_numpy(P.b, lb=P.origin)
    R.work = [F.empty_like(R.x) for _ in S.work]
    R.others = [] if P.w is None else [F.from_numpy(P.w, lb=P.origin)]
    R.minv = None if minv is None else F.from_numpy(minv, lb=P.origin)
    return R


def _solve(nh, S, P, entry, R, max_iters, tol2, check_every=CHECK_EVERY, dot="auto", region=None, trace=True):
    """-> (result of the solve, x, {name: work field} as numpy).  x is reset to x0 and the work fields are filled with NaN:
    the solver must not depend on what they hold."""
    R.x.tensor.copy_(nh.torch.from_numpy(np.ascontiguousarray(P.x0)))
    for f in R.work:
        f.tensor.fill_(float("nan"))
    res = S.solve(nh, entry, R.x, R.b, P.bounds, R.work, R.minv, R.others, max_iters, tol2, check_every=check_every, trace=trace,
                  dot=dot, region=region)
    nh.torch.cuda.synchronize()
    return res, R.x.numpy(), {nm: f.numpy() for nm, f in zip(S.work, R.work)}


def _device_minv(nh, S, P, entry, where, region):
    """PCG: the preconditioner apply.jacobi_minv builds on the device for Omega = bounds x region -- it must be the exact
    diagonal's, 1 / (4 rank + w) on Omega and 1 elsewhere -- ; the other solvers: None"""
    if not S.minv_needed:
        return None
    F = nh.fields.DeviceField
    like, w = F.from_numpy(P.x0, lb=P.origin), F.from_numpy(P.w, lb=P.origin)
    want = gc.numpy_minv(P.w, where)
    diag = nh.apply.operator_diagonal(entry, like, P.bounds, others=[w], region=region).numpy()
    assert bits_equal(diag, pc.diagonal(P.w, where)), mismatch_report(diag, pc.diagonal(P.w, where))
    got = nh.apply.jacobi_minv(entry, like, P.bounds, others=[w], region=region)
    assert bits_equal(got.numpy(), want), mismatch_report(got.numpy(), want)
    nh.keep.append(got)      # every preconditioner of this module stays allocated: two of them never share an address
    return want


def check_replay(nh, S, P, entry, iters, dot="auto", check_every=CHECK_EVERY, region=None, R=None, minv=None, claim_at=None,
                 label=""):
    """one traced solve of `iters` iterations against the replay of the definition on the problem's reference under `region`.
    minv: the preconditioner to solve with (default: the reference's own); claim_at: the iteration after which r . r must be
    below 1e-2 rr_0 (None: no claim).  -> (the fields used, x, the work fields, the trace)"""
    A, where, minv_ref = gc.restricted(P, region)
    minv = minv_ref if minv is None else minv
    R = _fields(nh, S, P, minv) if R is None else R
    (done, rr0, rr_last, trace), x, got = _solve(nh, S, P, entry, R, iters, 0.0, check_every=check_every, dot=dot, region=region)
    fused, fallback, checks = nh.apply.cg_counts()
    print(f"{S.name} {label} dot={dot}: fused {fused}, fallback {fallback}, checks {checks}")
    assert done == iters and trace.shape == (iters, len(S.scalars))
    assert fused + fallback == iters and checks == -(-iters // check_every)
    if dot == "fallback" and not isinstance(entry, int):
        assert (fused, fallback) == (0, iters)
    start = S.start(nh, rr0)
    _, start_refs = S.setup(P, A, where, minv)
    for nm, (ref, bound) in start_refs.items():
        print(f"  {nm} = {start[nm]!r} (terms' sum {ref!r}, bound {bound:.3e})")
        assert abs(start[nm] - ref) <= bound, nm
    want, refs = S.replay(P, A, where, minv, start, trace)
    for k, sums in enumerate(refs):
        print(f"  k={k}: " + "  ".join(f"{nm} = {trace[k][c]!r} (sum {s!r}, bound {bd:.3e})"
                                        for c, (nm, (s, bd)) in enumerate(zip(S.scalars, sums))))
        for c, (s, bd) in enumerate(sums):
            assert abs(float(trace[k][c]) - s) <= bd, (k, S.scalars[c])
    assert rr_last == float(trace[-1][S.rr_col])
    got["x"] = x
    for nm, ref in want.items():
        assert bits_equal(got[nm], ref), nm + ": " + mismatch_report(got[nm], ref)
    # cells of x outside Omega are never changed; the residual vectors are +0 there; no NaN is left in any work field
    outside = np.ones(P.shape, bool)
    outside[where] = False
    assert bits_equal(x[outside], P.x0[outside])
    zero = np.zeros(int(outside.sum()), P.dtype)
    for nm in S.zero_outside:
        assert bits_equal(got[nm][outside], zero), nm
    for nm in S.work:
        assert not np.isnan(got[nm]).any(), nm
    if claim_at is not None:
        at = min(iters, claim_at)
        assert float(trace[at - 1][S.rr_col]) < 1e-2 * rr0
    return R, x, got, trace


def check_nothing_to_solve(nh, S, P, entry, region, minv):
    """an empty Omega: nothing to iterate on, and forced iterations move nothing"""
    R = _fields(nh, S, P, minv)
    (done, rr0, rr_last, trace), x, got = _solve(nh, S, P, entry, R, 6, 0.0, region=region)
    assert (done, rr0, rr_last) == (0, 0.0, 0.0) and nh.apply.cg_counts() == (0, 0, 0) and trace.shape == (0, len(S.scalars))
    zero = np.zeros(P.shape, P.dtype)
    assert bits_equal(x, P.x0)
    for nm in S.zero_outside:
        assert bits_equal(got[nm], zero), nm
    # tol2 < 0 forces the iterations to run: every scalar is 0, so alpha = beta (= omega) = 0: nothing moves, nothing becomes NaN
    for dot in DOTS:
        (done, rr0, rr_last, trace), x, got = _solve(nh, S, P, entry, R, 3, -1.0, region=region, dot=dot)
        fused, fallback, checks = nh.apply.cg_counts()
        assert (done, rr0, rr_last) == (3, 0.0, 0.0) and fused + fallback == 3 and checks == 2
        assert bits_equal(trace, np.zeros((3, len(S.scalars)), P.dtype))
        assert bits_equal(x, P.x0)
        for nm in S.zero_outside:
            assert bits_equal(got[nm], zero), nm
        for nm in S.work:
            assert not np.isnan(got[nm]).any(), nm


@pytest.mark.parametrize("dot", DOTS)
@pytest.mark.parametrize("name,solver", gc.pairs([n for n in gc.CASES if n != gc.ZERO_TRIP]))
def test_replay_reproduces_every_vector_on_every_geometry(nh, name, solver, dot):
    S, P, case = gc.SOLVERS[solver], gc.problem(solver, name), gc.CASES[name]
    entry = _entry(nh, solver, name)
    minv = _device_minv(nh, S, P, entry, P.where, None)
    iters = gc.iters_of(solver, name)
    _, _, _, trace = check_replay(nh, S, P, entry, iters, dot=dot, minv=minv, claim_at=None if case.tiny else iters, label=name)
    if name == "r1_f32_3":
        # one unknown: the first iteration ends on r = +0 exactly, the second one runs on rr = 0 with alpha = beta = 0
        assert float(trace[0][S.rr_col]) == 0.0 and not trace[1].any()


@pytest.mark.parametrize("solver", list(gc.SOLVERS))
def test_zero_trip_bounds_leave_nothing_to_solve(nh, solver):
    S, P = gc.SOLVERS[solver], gc.problem(solver, gc.ZERO_TRIP)
    entry = _entry(nh, solver, gc.ZERO_TRIP)
    assert all(s.stop == s.start for s in P.where[:1])
    minv = _device_minv(nh, S, P, entry, P.where, None)
    if minv is not None:
        assert bits_equal(minv, np.ones(P.shape, P.dtype))
    check_nothing_to_solve(nh, S, P, entry, None, minv)


@pytest.mark.parametrize("dot", DOTS)
@pytest.mark.parametrize("solver", list(gc.SOLVERS))
@pytest.mark.parametrize("name", [n for n, (_, _, empty) in gc.REGIONS.items() if not empty])
def test_a_launch_region_restricts_omega_and_keeps_the_operators_result_zero_outside_it(nh, name, solver, dot):
    """Omega = bounds x region; the applies store nothing outside the region, where the solver keeps q (v and t) at +0: the
    reference is the oracle's operator masked to +0 out there"""
    case_name, region, _ = gc.REGIONS[name]
    S, P = gc.SOLVERS[solver], gc.problem(solver, case_name)
    entry = _entry(nh, solver, case_name)
    _, where, _ = gc.restricted(P, region)
    minv = _device_minv(nh, S, P, entry, where, region)
    iters = gc.iters_of(solver, name)
    check_replay(nh, S, P, entry, iters, dot=dot, region=region, minv=minv, claim_at=iters, label=name)


@pytest.mark.parametrize("solver", list(gc.SOLVERS))
def test_a_region_disjoint_from_the_bounds_leaves_nothing_to_solve(nh, solver):
    case_name, region, empty = gc.REGIONS["r3_disjoint"]
    S, P = gc.SOLVERS[solver], gc.problem(solver, case_name)
    entry = _entry(nh, solver, case_name)
    _, where, _ = gc.restricted(P, region)
    assert empty and any(s.stop <= s.start for s in where)
    minv = _device_minv(nh, S, P, entry, where, region)
    if minv is not None:
        assert bits_equal(minv, np.ones(P.shape, P.dtype))
    check_nothing_to_solve(nh, S, P, entry, region, minv)


@pytest.mark.parametrize("solver", list(gc.SOLVERS))
def test_a_cached_graph_is_not_replayed_under_another_region(nh, solver):
    """one entry, one set of fields, blocks of 10 iterations (long enough to be replayed from a captured graph): the whole box,
    then a dim-0 region, then the whole box again.  Each run is its own reference's; the first and the third are one run."""
    case_name, region, _ = gc.REGIONS[gc.GRAPH_REGION]
    S, P = gc.SOLVERS[solver], gc.problem(solver, case_name)
    entry = _entry(nh, solver, case_name)
    _, where, minv_region = gc.restricted(P, region)
    R = _fields(nh, S, P, P.minv)
    whole_minv = R.minv
    region_minv = None if minv_region is None else nh.fields.DeviceField.from_numpy(minv_region, lb=P.origin)
    claim_whole, claim_region = gc.iters_of(solver, case_name), gc.iters_of(solver, gc.GRAPH_REGION)
    _, x1, got1, trace1 = check_replay(nh, S, P, entry, 10, check_every=10, R=R, claim_at=claim_whole, label="whole box")
    R.minv = region_minv
    _, x2, _, _ = check_replay(nh, S, P, entry, 10, check_every=10, region=region, R=R, claim_at=claim_region, label="region")
    assert not bits_equal(x1, x2)
    R.minv = whole_minv
    _, x3, got3, trace3 = check_replay(nh, S, P, entry, 10, check_every=10, R=R, claim_at=claim_whole, label="whole box again")
    assert bits_equal(x1, x3) and bits_equal(trace1, trace3)
    for nm in S.zero_outside:
        assert bits_equal(got1[nm], got3[nm]), nm


@pytest.mark.parametrize("dot", DOTS)
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
@pytest.mark.parametrize("body", list(gc.BUILTIN))
def test_builtin_bodies_solve_through_their_own_launches(nh, body, solver, dot):
    """entry = a built-in body id: the solvers launch neptune_hip_apply_builtin and neptune_hip_apply_builtin_dot themselves,
    and the element type follows from the body.  (A built-in body always has a dot-monitored launch: dot="fallback" is the same
    request, and the fallback is taken only where that launch refuses.)  The bodies are no model problems: the replay, the
    scalar bounds, and r . r within the sqrt(2) of the numpy run's that the stop tests' thresholds rely on -- nothing else."""
    S, P = gc.SOLVERS[solver], gc.builtin_problem(body)
    entry = getattr(nh.capi, body)
    iters = gc.BUILTIN_ITERS
    seq = S.numpy(P, P.A, P.where, None, iters)
    _, _, _, trace = check_replay(nh, S, P, entry, iters, dot=dot, label=body)
    rr_last = float(trace[-1][S.rr_col])
    print(f"  rr_last = {rr_last!r}, numpy {seq[iters]!r}")
    assert seq[iters] / math.sqrt(2.0) <= rr_last <= seq[iters] * math.sqrt(2.0)


# ---------------------------------------------------------------- the folded set-up grid
FOLDED_SHAPE = (2049, 2049, 3)        # 2049 * 2049 rows of one 256-cell chunk: 4 198 401 workgroups, more than 2^22


@pytest.fixture(scope="module")
def folded():
    """b integer-valued in [-3, 3], minv per cell from {0.25, 0.5, 1}: every term of r . r and r . (minv r) is a small dyadic
    number and every partial sum is exact, whatever the tree"""
    class D:
        pass
    d = D()
    h = helpers.hash_field(FOLDED_SHAPE, np.float64, seed=71)
    d.b = np.rint(3.0 * h) + 0.0          # no -0: b - A(0) is then b whatever the sign of the operator's zero
    assert d.b.min() == -3.0 and d.b.max() == 3.0
    d.minv = pc.w_field(FOLDED_SHAPE, np.float64, seed=73, values=(0.25, 0.5, 1.0))
    d.where = tuple(slice(1, n - 1) for n in FOLDED_SHAPE)
    d.r = np.zeros(FOLDED_SHAPE)
    d.r[d.where] = d.b[d.where]
    d.rr0 = float(np.sum(d.r.astype(np.int64) ** 2))
    d.rz0 = float(np.sum(np.rint(4.0 * d.minv * d.r * d.r).astype(np.int64))) / 4.0
    assert d.rr0 < 2.0 ** 53 and d.rz0 < 2.0 ** 51
    return d


@pytest.mark.parametrize("solver", list(gc.SOLVERS))
def test_the_set_up_on_a_grid_folded_into_two_dimensions_sums_exactly(nh, folded, solver):
    """max_iters = 0: the set-up alone, on a box whose rows outnumber the 2^22 workgroups of one grid dimension -- the set-up
    kernels then run on a two-dimensional grid whose last row of workgroups owns no cell, and the second sum's partials start
    behind ALL of the grid's workgroups.  x0 = 0, so A(x0) = 0 and r = b on Omega: rr_0 and rz_0 are sums of exact terms and
    must EQUAL the integer sums."""
    S, F, torch = gc.SOLVERS[solver], nh.fields.DeviceField, nh.torch
    shape = FOLDED_SHAPE
    bounds = ([1, 1, 1], [n - 1 for n in shape])
    x, b = F.from_numpy(np.zeros(shape)), F.from_numpy(folded.b)
    work = [F.empty_like(x) for _ in S.work]
    for f in work:
        f.tensor.fill_(float("nan"))
    minv = F.from_numpy(folded.minv) if S.minv_needed else None
    try:
        done, rr0, rr_last = S.solve(nh, nh.capi.BODY_LAP3D7_F64, x, b, bounds, work, minv, [], 0, 0.0, trace=False)
        torch.cuda.synchronize()
        assert (done, rr_last) == (0, rr0) and nh.apply.cg_counts() == (0, 0, 0)
        print(f"{solver}: rr0 = {rr0!r} (exact {folded.rr0!r})")
        assert rr0 == folded.rr0
        got = {nm: f.numpy() for nm, f in zip(S.work, work)}
        assert bits_equal(got["r"], folded.r), mismatch_report(got["r"], folded.r)
        if S.minv_needed:
            rz0 = nh.apply.pcg_rz0()
            print(f"  rz0 = {rz0!r} (exact {folded.rz0!r})")
            assert rz0 == folded.rz0
            want_p = np.zeros(shape)
            want_p[folded.where] = folded.minv[folded.where] * folded.r[folded.where]
            assert bits_equal(got["p"], want_p), mismatch_report(got["p"], want_p)
        else:
            assert bits_equal(got["p"], folded.r), mismatch_report(got["p"], folded.r)
        if "rh" in got:
            assert bits_equal(got["rh"], folded.r), mismatch_report(got["rh"], folded.r)
        assert not x.tensor.any()
    finally:
        del x, b, work, minv
        torch.cuda.empty_cache()
