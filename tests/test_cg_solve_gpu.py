"""neptune_hip_cg_solve: conjugate gradients whose vectors and scalars stay on the device.

Operator: cg_cases.cg_module -- d * centre - (star neighbours), d = 12 (7-point) or 24 (radius 2), copy-through on the rim:
symmetric positive definite on the interior with condition number at most 3, so r . r falls by about an order of magnitude
per iteration.

Replay: the solver keeps a trace of its device scalars (pq_k, rr_(k+1)).  cg_cases.replay runs the recurrences of the
definition in numpy with alpha_k and beta_k formed from THOSE scalars (one division each, in the element type) and q from
the oracle's operator; whatever order the device summed in, x, r and p must then agree bit for bit, and each traced scalar
must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the replay's own terms.

Stop: thresholds sit at the geometric mean of two consecutive check values of a numpy run of the same recurrences, which the
test first requires to differ by a factor of 2 -- four orders (f32) to thirteen (f64) above what two summation orders move
r . r by over 13 iterations -- so the iteration count follows from the definition alone."""
import ctypes as C
import math

import numpy as np
import pytest

import cg_cases as cc
import helpers
import solver_trace_cases as stc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

NUMPY_ITERS = 13
# name: (shape, dtype, radius, non-zero rim values in x)
PROBLEMS = {
    "f64_12x20x136": ((12, 20, 136), np.float64, 1, False),
    "f32_12x20x136": ((12, 20, 136), np.float32, 1, False),
    "f64_9x11x131_rim": ((9, 11, 131), np.float64, 1, True),
    "f32_9x11x131": ((9, 11, 131), np.float32, 1, False),             # n % 4 == 1: the f32 tail of the 16-byte kernels
    "f64_8x512x520": ((8, 512, 520), np.float64, 1, False),         # 2 129 920 cells: past the 2 097 152 lanes of the capped grid
    "f64_12x20x136_radius2": ((12, 20, 136), np.float64, 2, False),   # held to the plane-in-LDS kernel by PLANE_TILE
}
PLANE_TILE = 7
BIG = "f64_8x512x520"


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
    ns.cache = {}
    return ns


class Problem:
    pass


def _problem(nh, name):
    """the compiled operator, its oracle, x0 / b and the numpy run's r . r sequence: computed once per problem, left unchanged"""
    if name not in nh.cache:
        shape, dtype, radius, rim = PROBLEMS[name]
        P = Problem()
        P.shape, P.dtype, P.radius = shape, dtype, radius
        text = cc.cg_module(shape, dtype, radius=radius)
        P.entry = nh.lowering.compile_module(text, dot_entries=True).dot_entry("entry")
        P.A = cc.Operator(text)
        P.bounds = cc.interior(shape, radius)
        P.where = tuple(slice(radius, n - radius) for n in shape)
        P.b = helpers.hash_field(shape, dtype, seed=71)
        P.x0 = helpers.hash_field(shape, dtype, seed=72) if rim else np.zeros(shape, dtype)
        P.seq = cc.numpy_cg(P.A, P.x0, P.b, P.where, NUMPY_ITERS) if name != BIG else None
        for a in (P.b, P.x0):
            a.setflags(write=False)
        nh.cache[name] = P
    return nh.cache[name]


def _solve(nh, P, max_iters, tol2, check_every=1, trace=False, dot="auto", cfg=None, x0=None, b=None, offset=0):
    F = nh.fields.DeviceField
    make = (lambda a: stc.offset_field(nh, a, offset)) if offset else F.from_numpy
    x = make(P.x0 if x0 is None else x0)
    bf = make(P.b if b is None else b)
    work = [make(np.full(P.shape, np.nan, P.dtype)) for _ in range(3)]    # the solver must not depend on what the work fields hold
    res = nh.apply.cg_solve(P.entry, x, bf, P.bounds, max_iters, tol2, check_every=check_every, trace=trace, dot=dot, cfg=cfg,
                            work=work)
    nh.torch.cuda.synchronize()
    return res, x.numpy(), [w.numpy() for w in work]


def _check_replay(nh, name, iters, check_every, dot="auto", cfg=None, path="fused", offset=0, solves=True):
    P = _problem(nh, name)
    (done, rr0, rr_last, trace), x, (r, p, q) = _solve(nh, P, iters, 0.0, check_every=check_every, trace=True, dot=dot, cfg=cfg,
                                                       offset=offset)
    fused, fallback, checks = nh.apply.cg_counts()
    assert done == iters and trace.shape == (iters, 2)
    assert checks == -(-iters // check_every)
    assert (fused, fallback) == ((iters, 0) if path == "fused" else (0, iters))
    _, _, (rr0_ref, rr0_bound) = cc.setup(P.A, P.x0, P.b, P.where)
    print(f"{name} {path}: rr0 = {rr0!r} (terms' sum {rr0_ref!r}, bound {rr0_bound:.3e})")
    assert abs(rr0 - rr0_ref) <= rr0_bound
    xr, rr_, pr, refs = cc.replay(P.A, P.x0, P.b, P.where, rr0, trace)
    for k, ((pq_ref, pq_bound), (rr_ref, rr_bound)) in enumerate(refs):
        print(f"  k={k}: pq = {trace[k][0]!r} (sum {pq_ref!r}, bound {pq_bound:.3e})  rr' = {trace[k][1]!r} "
              f"(sum {rr_ref!r}, bound {rr_bound:.3e})")
        assert abs(float(trace[k][0]) - pq_ref) <= pq_bound and abs(float(trace[k][1]) - rr_ref) <= rr_bound
    assert rr_last == float(trace[-1][1])
    assert bits_equal(x, xr), mismatch_report(x, xr)
    assert bits_equal(r, rr_), mismatch_report(r, rr_)
    assert bits_equal(p, pr), mismatch_report(p, pr)
    # cells of x outside Omega are never written; r and p are +0 there
    outside = np.ones(P.shape, bool)
    outside[P.where] = False
    assert bits_equal(x[outside], P.x0[outside])
    zero = np.zeros(int(outside.sum()), P.dtype)
    assert bits_equal(r[outside], zero) and bits_equal(p[outside], zero)
    # ... and it is a solve: the residual has fallen as the numpy run's has
    if solves:
        assert rr_last <= 4.0 * P.seq[iters] and P.seq[iters] < 1e-3 * P.seq[0]


@pytest.mark.parametrize("name,iters", [("f64_12x20x136", 8), ("f32_12x20x136", 6), ("f64_9x11x131_rim", 8), ("f32_9x11x131", 6)])
def test_replay_from_the_traced_scalars_reproduces_every_vector(nh, name, iters):
    _check_replay(nh, name, iters, check_every=1)


def test_fields_at_an_8_byte_offset_run_the_scalar_kernel_forms(nh):
    """x, b, r, p, q one f64 element into larger allocations: not 16-byte aligned, so the grid-stride forms of the update and
    direction kernels run"""
    _check_replay(nh, "f64_9x11x131_rim", 8, check_every=3, offset=1)


def test_more_cells_than_lanes_take_the_grid_stride_loops_round_again(nh):
    """2 129 920 cells in fields one element off 16-byte alignment: the scalar forms' grid is capped at 256 * 32 workgroups
    (2 097 152 lanes), so 32 768 lanes make a second trip.  Two iterations: a wrong stride, or a cell summed twice, shows in
    the vectors and in rr'.  (Too few iterations for the convergence check of the small problems.)"""
    _check_replay(nh, BIG, 2, check_every=2, offset=1, solves=False)


def test_a_block_long_enough_to_be_replayed_as_a_graph(nh):
    """one block of 10 iterations: the first one plain, eight from a captured graph, one plain"""
    _check_replay(nh, "f64_12x20x136", 10, check_every=10)


@pytest.mark.parametrize("name", ["f64_12x20x136", "f32_12x20x136"])
@pytest.mark.parametrize("check_every,max_iters", [(1, 13), (3, 13), (3, 8)])
def test_stops_where_the_definition_stops(nh, name, check_every, max_iters):
    P = _problem(nh, name)
    # between the check values number 2 and 3; with max_iters = 8 the third block is cut short (3 + 3 + 2) and the threshold
    # sits below it, so the loop runs to max_iters
    if max_iters == 8:
        tol2 = cc.tol_between(P.seq, 8, 9)
    else:
        tol2 = cc.tol_between(P.seq, 2 * check_every, 3 * check_every)
    want_done, want_checks = cc.expected_stop(P.seq, check_every, max_iters, tol2)
    assert want_done == (8 if max_iters == 8 else 3 * check_every) and want_checks == 3
    (done, rr0, rr_last), _, _ = _solve(nh, P, max_iters, tol2, check_every=check_every)
    fused, fallback, checks = nh.apply.cg_counts()
    print(f"{name} check_every={check_every} max_iters={max_iters}: iters={done} rr0={rr0!r} rr_last={rr_last!r} numpy {P.seq[done]!r}")
    assert done == want_done and checks == want_checks and (fused, fallback) == (done, 0)
    assert (rr_last <= tol2) == (P.seq[done] <= tol2)
    # two summation orders (numpy's pairwise and a serial one) move r . r of this run by at most 7e-14 (f64) and 5e-5 (f32)
    # relative over 13 iterations; the device's tree is a third order: 1e-3 leaves a factor of 20
    assert abs(rr_last - P.seq[done]) <= 1e-3 * P.seq[done]


def test_initial_residual_below_the_threshold_runs_no_iteration(nh):
    P = _problem(nh, "f64_9x11x131_rim")
    (done, rr0, rr_last), x, (r, p, q) = _solve(nh, P, 10, 2.0 * P.seq[0])
    assert done == 0 and rr0 == rr_last and abs(rr0 - P.seq[0]) <= 1e-12 * P.seq[0] and nh.apply.cg_counts() == (0, 0, 0)
    assert bits_equal(x, P.x0)
    # max_iters = 0: the set-up alone
    (done, rr0b, _), x, _ = _solve(nh, P, 0, 0.0)
    assert done == 0 and rr0b == rr0 and bits_equal(x, P.x0)


@pytest.mark.parametrize("name,dot,tile", [("f64_12x20x136", "fallback", None), ("f64_9x11x131_rim", "fallback", None),
                                           ("f64_12x20x136_radius2", "auto", PLANE_TILE)])
def test_fallback_runs_the_same_iteration(nh, name, dot, tile):
    cfg = None if tile is None else nh.apply.make_cfg(nh.capi.KERNEL_MARCH, tile)
    _check_replay(nh, name, 8, check_every=3, dot=dot, cfg=cfg, path="fallback")
    # the iteration count under a threshold is the fused path's / the definition's
    P = _problem(nh, name)
    tol2 = cc.tol_between(P.seq, 4, 5)
    (done, _, _), _, _ = _solve(nh, P, NUMPY_ITERS, tol2, dot=dot, cfg=cfg)
    assert done == 5 and nh.apply.cg_counts() == (0, 5, 5)
    if tile is None:
        (done_fused, _, _), _, _ = _solve(nh, P, NUMPY_ITERS, tol2)
        assert done_fused == 5 and nh.apply.cg_counts() == (5, 0, 5)


def test_exact_breakdown_leaves_everything_as_it_is(nh):
    P = _problem(nh, "f64_9x11x131_rim")
    b = P.A(P.x0)                      # b = A(x) exactly: the residual is +0 everywhere
    (done, rr0, rr_last), x, _ = _solve(nh, P, 5, 0.0, b=b)
    assert (done, rr0, rr_last) == (0, 0.0, 0.0)
    # tol2 < 0 forces the iterations to run: alpha = beta = 0, nothing moves, nothing becomes NaN
    (done, rr0, rr_last, trace), x, (r, p, q) = _solve(nh, P, 3, -1.0, trace=True, b=b)
    assert (done, rr0, rr_last) == (3, 0.0, 0.0) and nh.apply.cg_counts() == (3, 0, 3)
    assert bits_equal(x, P.x0)
    zero = np.zeros(P.shape, P.dtype)
    assert bits_equal(r, zero) and bits_equal(p, zero) and np.isfinite(q).all()
    assert bits_equal(trace, np.zeros((3, 2), P.dtype))


def test_refusals_launch_nothing(nh):
    P = _problem(nh, "f64_12x20x136")
    F = nh.fields.DeviceField
    x, b = F.from_numpy(P.x0), F.from_numpy(P.b)
    work = [F.empty_like(x) for _ in range(3)]
    x.tensor.fill_(-3.0)
    for w in work:
        w.tensor.fill_(-5.0)
    g = nh.apply.geom_for([x], work[2], P.bounds)
    n_bytes = x.tensor.numel() * 8
    trace = nh.torch.full((2 * 8,), -7.0, dtype=nh.torch.float64, device="cuda")
    st = nh.fields.current_stream_ptr()

    def call(xp=x.ptr, bp=b.ptr, w=None, max_iters=8, check_every=1, tr=None, stream=st):
        w = [f.ptr for f in work] if w is None else w
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = nh.lib.neptune_hip_cg_solve(C.cast(P.entry.fn, C.c_void_p), C.cast(P.entry.fn_dot, C.c_void_p), -1, x.dtype, C.byref(g),
                                         xp, bp, (C.c_void_p * 3)(*w), None, max_iters, check_every, 1e-30, tr, stream, None,
                                         C.byref(done), C.byref(rr0), C.byref(last))
        return rc, done.value
    E = nh.capi.EINVAL
    assert call(check_every=0) == (E, 0)
    assert call(max_iters=-1) == (E, 0)
    assert call(xp=None) == (E, 0) and call(bp=None) == (E, 0)
    assert call(w=[work[0].ptr, None, work[2].ptr]) == (E, 0)                       # a null work field
    assert call(bp=x.ptr) == (E, 0)                                                 # x and b are one buffer
    assert call(w=[work[0].ptr, work[0].ptr + 64, work[2].ptr]) == (E, 0)           # r and p overlap
    assert call(w=[work[0].ptr, work[1].ptr, x.ptr + n_bytes - 8]) == (E, 0)        # q starts in x's last cell
    assert call(tr=work[1].ptr + 16) == (E, 0)                                      # a trace inside p
    assert call(tr=trace.data_ptr() , w=[work[0].ptr, work[1].ptr, trace.data_ptr()]) == (E, 0)
    # a call while the stream is being captured: rr could not be read back
    torch = nh.torch
    side = torch.cuda.Stream()
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        scratch.add_(1.0)
        captured = call(stream=int(side.cuda_stream))
    assert captured == (E, 0)
    torch.cuda.synchronize()
    assert bool((x.tensor == -3.0).all()) and all(bool((w.tensor == -5.0).all()) for w in work)
    assert bool((trace == -7.0).all()) and bits_equal(b.numpy(), P.b)
