"""neptune_hip_bicgstab_solve: BiCGStab whose vectors and scalars stay on the device.

Operator: bicg_cases.bicg_module -- a 7-point upwind advection-diffusion operator, not symmetric; plain CG diverges on it
(tests/test_bicg_host.py).

Replay: the solver keeps a trace of its device scalars (rv_k, ts_k, tt_k, rho_(k+1), rr_(k+1)).  bicg_cases.replay runs the
recurrences of the definition in numpy with alpha_k, omega_k and beta_k formed from THOSE scalars (the stated divisions, in
the element type) and v, t from the oracle's operator; whatever order the device summed in, x, r and p must then agree bit for
bit, and each traced scalar must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the replay's own terms.

Stop: BiCGStab's r . r is not monotone, so thresholds sit at bicg_cases.stop_points of a numpy run of the same recurrences: the
geometric mean of a value and the minimum of all earlier ones, which differ by a factor of 2 at least.  Only points among the
first six iterations are used: there the numpy run falls steadily (its first rise is at iteration 7), and two summation
orders move r . r by parts in 1e13 (f64) / 1e5 (f32), so the iteration count follows from the definition alone."""
import ctypes as C
import math

import numpy as np
import pytest

import bicg_cases as bc
import cg_cases as cc
import helpers
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

NUMPY_ITERS = 12
SCALARS = ("rv", "ts", "tt", "rho'", "rr'")
# name: (shape, dtype, operator, non-zero rim values in x)
PROBLEMS = {
    "f64_12x20x136": ((12, 20, 136), np.float64, "upwind", False),
    "f32_12x20x136": ((12, 20, 136), np.float32, "upwind", False),
    "f64_9x11x131_rim": ((9, 11, 131), np.float64, "upwind", True),
    "f32_9x11x131": ((9, 11, 131), np.float32, "upwind", False),               # n % 4 == 1: the f32 tail of the 16-byte kernels
    "f64_8x512x520": ((8, 512, 520), np.float64, "upwind", False),         # 2 129 920 cells: past the 2 097 152 lanes of the capped grid
    "f64_12x20x136_radius2": ((12, 20, 136), np.float64, "spd_radius2", False),   # held to the plane-in-LDS kernel by PLANE_TILE
}
PLANE_TILE = 7
CG_SHAPE = (12, 20, 136)
BIG = "f64_8x512x520"


def _cg_run(ns):
    """cg_solve on cg_cases' problem: -> (result, x, r, p) with the trace"""
    F = ns.fields.DeviceField
    if "cg" not in ns.cache:
        text = cc.cg_module(CG_SHAPE, np.float64)
        ns.cache["cg"] = (ns.lowering.compile_module(text, dot_entries=True).dot_entry("entry"),
                          helpers.hash_field(CG_SHAPE, np.float64, seed=71))
    entry, b = ns.cache["cg"]
    x, bf = F.from_numpy(np.zeros(CG_SHAPE, np.float64)), F.from_numpy(b)
    work = [F.empty_like(x) for _ in range(3)]
    for w in work:
        w.tensor.fill_(float("nan"))
    res = ns.apply.cg_solve(entry, x, bf, cc.interior(CG_SHAPE), 10, 0.0, check_every=10, trace=True, work=work)
    ns.torch.cuda.synchronize()
    return res, x.numpy(), work[0].numpy(), work[1].numpy()


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
    # before this module's first BiCGStab call (no other module makes one): what test_cg_solve_is_unchanged compares with
    ns.cg_before = _cg_run(ns)
    return ns


class Problem:
    pass


def _problem(nh, name):
    """the compiled operator, its oracle, x0 / b and the numpy run's r . r sequence: computed once per problem, left unchanged"""
    if name not in nh.cache:
        shape, dtype, op, rim = PROBLEMS[name]
        P = Problem()
        P.shape, P.dtype = shape, dtype
        radius = 2 if op == "spd_radius2" else 1
        text = cc.cg_module(shape, dtype, radius=2) if op == "spd_radius2" else bc.bicg_module(shape, dtype)
        P.entry = nh.lowering.compile_module(text, dot_entries=True).dot_entry("entry")
        P.A = bc.Operator(text)
        P.bounds = cc.interior(shape, radius)
        P.where = tuple(slice(radius, n - radius) for n in shape)
        P.b = helpers.hash_field(shape, dtype, seed=71)
        P.x0 = helpers.hash_field(shape, dtype, seed=72) if rim else np.zeros(shape, dtype)
        P.seq = bc.numpy_bicgstab(P.A, P.x0, P.b, P.where, NUMPY_ITERS) if name != BIG else None
        for a in (P.b, P.x0):
            a.setflags(write=False)
        nh.cache[name] = P
    return nh.cache[name]


def _offset_field(nh, a, elems):
    """a field holding `a` that starts `elems` elements into a larger allocation"""
    dtype = nh.fields._FROM_NP[a.dtype]
    big = nh.torch.empty(a.size + elems, dtype=nh.fields._TORCH_DTYPE[dtype], device="cuda")
    view = big[elems:].view(a.shape)
    view.copy_(nh.torch.from_numpy(np.ascontiguousarray(a)))
    f = nh.fields.DeviceField((0,) * a.ndim, a.shape, dtype, view)
    assert f.ptr == big.data_ptr() + elems * a.itemsize
    return f


def _solve(nh, P, max_iters, tol2, check_every=1, trace=False, dot="auto", cfg=None, x0=None, b=None, offset=0, region=None,
           fields=None):
    """-> (result of bicgstab_solve, x, [r, rh, p, v, t] as numpy, the device fields used).  The work fields are pre-filled
    with NaN: the solver must not depend on what they hold.  fields: the (x, b, work) of an earlier call, used again."""
    F = nh.fields.DeviceField
    make = (lambda a: _offset_field(nh, a, offset)) if offset else F.from_numpy
    nan = np.full(P.shape, np.nan, P.dtype)
    if fields is None:
        x, bf, work = make(P.x0 if x0 is None else x0), make(P.b if b is None else b), [make(nan) for _ in range(5)]
    else:
        x, bf, work = fields
        x.tensor.copy_(nh.torch.from_numpy(np.ascontiguousarray(P.x0 if x0 is None else x0)))
        for f in work:
            f.tensor.fill_(float("nan"))
    res = nh.apply.bicgstab_solve(P.entry, x, bf, P.bounds, max_iters, tol2, check_every=check_every, trace=trace, dot=dot,
                                  cfg=cfg, work=work, region=region)
    nh.torch.cuda.synchronize()
    return res, x.numpy(), [f.numpy() for f in work], (x, bf, work)


def _check_replay(nh, name, iters, check_every, dot="auto", cfg=None, path="fused", offset=0, region=None, fields=None,
                  solves=True):
    P = _problem(nh, name)
    (done, rr0, rr_last, trace), x, (r, rh, p, v, t), used = _solve(nh, P, iters, 0.0, check_every=check_every, trace=True,
                                                                   dot=dot, cfg=cfg, offset=offset, region=region, fields=fields)
    fused, fallback, checks = nh.apply.cg_counts()
    assert done == iters and trace.shape == (iters, 5)
    assert checks == -(-iters // check_every)
    assert (fused, fallback) == ((iters, 0) if path == "fused" else (0, iters))
    # Omega = bounds x launch region; outside the region an apply stores nothing and the solver keeps v and t at +0
    where, A = P.where, P.A
    if region is not None:
        where = tuple(slice(max(w.start, lo), min(w.stop, hi)) for w, lo, hi in zip(P.where, *region))
        inside = np.zeros(P.shape, bool)
        inside[tuple(slice(lo, hi) for lo, hi in zip(*region))] = True

        def A(u):
            return np.where(inside, P.A(u), P.dtype(0))
    r0, _, _, (rr0_ref, rr0_bound) = bc.setup(A, P.x0, P.b, where)
    print(f"{name} {path}: rr0 = {rr0!r} (terms' sum {rr0_ref!r}, bound {rr0_bound:.3e})")
    assert abs(rr0 - rr0_ref) <= rr0_bound
    xr, rr_, pr, refs = bc.replay(A, P.x0, P.b, where, rr0, trace)
    for k, sums in enumerate(refs):
        print(f"  k={k}: " + "  ".join(f"{nm} = {trace[k][c]!r} (sum {s!r}, bound {bd:.3e})"
                                        for c, (nm, (s, bd)) in enumerate(zip(SCALARS, sums))))
        for c, (s, bd) in enumerate(sums):
            assert abs(float(trace[k][c]) - s) <= bd, (k, SCALARS[c])
    assert rr_last == float(trace[-1][4])
    assert bits_equal(x, xr), mismatch_report(x, xr)
    assert bits_equal(r, rr_), mismatch_report(r, rr_)
    assert bits_equal(p, pr), mismatch_report(p, pr)
    assert bits_equal(rh, r0), mismatch_report(rh, r0)
    # cells of x outside Omega are never changed; r, rh and p are +0 there; nothing of the NaN the work fields held is left
    outside = np.ones(P.shape, bool)
    outside[where] = False
    assert bits_equal(x[outside], P.x0[outside])
    zero = np.zeros(int(outside.sum()), P.dtype)
    assert bits_equal(r[outside], zero) and bits_equal(rh[outside], zero) and bits_equal(p[outside], zero)
    assert np.isfinite(v).all() and np.isfinite(t).all()
    # ... and it is a solve: after min(iters, 6) iterations -- where the numpy run still falls steadily -- r . r is below
    # 1e-2 rr_0 (the numpy runs are at 2e-4 and below, tests/test_bicg_host.py), and on the numpy run's own problem within the
    # sqrt(2) of it that the stop tests' thresholds rely on
    at = min(iters, 6)
    rr_at = float(trace[at - 1][4])
    if not solves:
        return used, x, r, p, trace
    assert rr_at < 1e-2 * rr0
    if region is None:
        assert P.seq[at] / math.sqrt(2.0) <= rr_at <= P.seq[at] * math.sqrt(2.0)
    return used, x, r, p, trace


@pytest.mark.parametrize("name,iters", [("f64_12x20x136", 8), ("f32_12x20x136", 6), ("f64_9x11x131_rim", 8), ("f32_9x11x131", 6)])
def test_replay_from_the_traced_scalars_reproduces_every_vector(nh, name, iters):
    _check_replay(nh, name, iters, check_every=1)


def test_more_cells_than_lanes_take_the_grid_stride_loops_round_again(nh):
    """2 129 920 cells in fields one element off 16-byte alignment: the scalar forms' grid is capped at 256 * 32 workgroups
    (2 097 152 lanes), so 32 768 lanes make a second trip.  Two iterations: a wrong stride, or a cell summed twice, shows in
    the vectors and in all five sums.  (Too few iterations for the convergence check of the small problems.)"""
    _check_replay(nh, BIG, 2, check_every=2, offset=1, solves=False)


def test_fields_at_an_8_byte_offset_run_the_scalar_kernel_forms(nh):
    """all seven fields one f64 element into larger allocations: not 16-byte aligned, so the grid-stride forms of the flat
    kernels run"""
    _check_replay(nh, "f64_9x11x131_rim", 8, check_every=3, offset=1)


def test_a_launch_region_keeps_v_and_t_zero_outside_it(nh):
    """a launch region restricted along dim 0: Omega shrinks, the applies store nothing outside the region, and the flat kernels
    read the +0 the solver put into v and t there (the work fields start as NaN)"""
    P = _problem(nh, "f64_9x11x131_rim")
    region = ([2, 0, 0], [7, P.shape[1], P.shape[2]])
    _check_replay(nh, "f64_9x11x131_rim", 6, check_every=2, region=region)


def test_a_block_replayed_as_a_graph_gives_the_same_bits_twice(nh):
    """one block of 10 iterations: the first one plain, two captured graphs of four, one plain; then the same call on the same
    fields again, which replays the cached graph"""
    name = "f64_12x20x136"
    used, x1, r1, p1, trace1 = _check_replay(nh, name, 10, check_every=10)
    _, x2, r2, p2, trace2 = _check_replay(nh, name, 10, check_every=10, fields=used)
    assert bits_equal(x1, x2) and bits_equal(r1, r2) and bits_equal(p1, p2) and bits_equal(trace1, trace2)


@pytest.mark.parametrize("name", ["f64_12x20x136", "f32_12x20x136"])
@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("dot", ["auto", "fallback"])
def test_stops_where_the_definition_stops(nh, name, check_every, dot):
    P = _problem(nh, name)
    # the last stop point among the first six iterations that a check falls on
    points = [(k, tol2) for k, tol2 in bc.stop_points(P.seq, 6) if k % check_every == 0]
    assert points, "precondition (tests/test_bicg_host.py): stop points among the first iterations"
    k, tol2 = points[-1]
    assert k >= 3
    want_done, want_checks = bc.expected_stop(P.seq, check_every, NUMPY_ITERS, tol2)
    assert (want_done, want_checks) == (k, k // check_every)
    (done, rr0, rr_last), _, _, _ = _solve(nh, P, NUMPY_ITERS, tol2, check_every=check_every, dot=dot)
    fused, fallback, checks = nh.apply.cg_counts()
    print(f"{name} check_every={check_every} {dot}: iters={done} rr0={rr0!r} rr_last={rr_last!r} numpy {P.seq[done]!r} tol2={tol2!r}")
    assert done == want_done and checks == want_checks
    assert (fused, fallback) == ((done, 0) if dot == "auto" else (0, done))
    assert rr_last <= tol2
    # what the threshold's place relies on: the device's r . r within sqrt(2) of the numpy run's
    assert P.seq[done] / math.sqrt(2.0) <= rr_last <= P.seq[done] * math.sqrt(2.0)


def test_initial_residual_below_the_threshold_runs_no_iteration(nh):
    P = _problem(nh, "f64_9x11x131_rim")
    (done, rr0, rr_last), x, _, _ = _solve(nh, P, 10, 2.0 * P.seq[0])
    assert done == 0 and rr0 == rr_last and abs(rr0 - P.seq[0]) <= 1e-12 * P.seq[0] and nh.apply.cg_counts() == (0, 0, 0)
    assert bits_equal(x, P.x0)
    # max_iters = 0: the set-up alone
    (done, rr0b, _), x, _, _ = _solve(nh, P, 0, 0.0)
    assert done == 0 and rr0b == rr0 and bits_equal(x, P.x0)


@pytest.mark.parametrize("name,dot,tile", [("f64_12x20x136", "fallback", None), ("f64_9x11x131_rim", "fallback", None),
                                           ("f64_12x20x136_radius2", "auto", PLANE_TILE)])
def test_fallback_runs_the_same_iteration(nh, name, dot, tile):
    """dot="fallback", and a dot entry that refuses (a radius-2 operator held to the plane-in-LDS kernel): step 3 is a plain
    launch and ONE pass that forms ts and tt"""
    cfg = None if tile is None else nh.apply.make_cfg(nh.capi.KERNEL_MARCH, tile)
    _check_replay(nh, name, 8 if tile is None else 5, check_every=3, dot=dot, cfg=cfg, path="fallback")


def test_exact_breakdown_leaves_everything_as_it_is(nh):
    P = _problem(nh, "f64_9x11x131_rim")
    F = nh.fields.DeviceField
    # b = A(x0) by the device's own plain launch: the residual is +0 everywhere on Omega, exactly
    xf = F.from_numpy(P.x0)
    out = F.empty_like(xf)
    nh.apply.apply_builtin(P.entry, [xf], out, P.bounds)
    nh.torch.cuda.synchronize()
    b = out.numpy()
    (done, rr0, rr_last), x, _, _ = _solve(nh, P, 5, 0.0, b=b)
    assert (done, rr0, rr_last) == (0, 0.0, 0.0) and nh.apply.cg_counts() == (0, 0, 0)
    assert bits_equal(x, P.x0)
    # tol2 < 0 forces the iterations to run: alpha = omega = beta = 0, nothing moves, nothing becomes NaN
    (done, rr0, rr_last, trace), x, work, _ = _solve(nh, P, 3, -1.0, trace=True, b=b)
    assert (done, rr0, rr_last) == (3, 0.0, 0.0) and nh.apply.cg_counts() == (3, 0, 3)
    assert bits_equal(x[P.where], P.x0[P.where]) and bits_equal(x, P.x0)
    zero = np.zeros(P.shape, P.dtype)
    r, rh, p, v, t = work
    assert bits_equal(r, zero) and bits_equal(rh, zero) and bits_equal(p, zero)
    assert all(np.isfinite(w).all() for w in work)
    assert bits_equal(trace, np.zeros((3, 5), P.dtype))


def test_refusals_launch_nothing(nh):
    P = _problem(nh, "f64_12x20x136")
    F = nh.fields.DeviceField
    x, b = F.from_numpy(P.x0), F.from_numpy(P.b)
    work = [F.empty_like(x) for _ in range(5)]
    x.tensor.fill_(-3.0)
    for w in work:
        w.tensor.fill_(-5.0)
    g = nh.apply.geom_for([x], work[3], P.bounds)
    n_bytes = x.tensor.numel() * 8
    trace = nh.torch.full((5 * 8 + 16,), -7.0, dtype=nh.torch.float64, device="cuda")
    st = nh.fields.current_stream_ptr()
    seven = [x.ptr, b.ptr] + [f.ptr for f in work]

    def call(f=None, max_iters=8, check_every=1, tr=None, stream=st):
        f = seven if f is None else f
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = nh.lib.neptune_hip_bicgstab_solve(C.cast(P.entry.fn, C.c_void_p), C.cast(P.entry.fn_dot, C.c_void_p), -1, x.dtype,
                                               C.byref(g), f[0], f[1], (C.c_void_p * 5)(*f[2:]), None, max_iters, check_every,
                                               1e-30, tr, stream, None, C.byref(done), C.byref(rr0), C.byref(last))
        return rc, done.value

    def swapped(i, value):
        f = list(seven)
        f[i] = value
        return f
    E = nh.capi.EINVAL
    assert call(check_every=0) == (E, 0)
    assert call(max_iters=-1) == (E, 0)
    for i in range(7):
        assert call(f=swapped(i, None)) == (E, 0)                                   # a null field
        assert call(f=swapped(i, seven[i] + 4)) == (E, 0)                           # misaligned for f64
        assert call(tr=seven[i] + 16) == (E, 0)                                     # a trace inside the field
        # the trace is 5 * max_iters = 40 values long: used as a field, a pointer 39 values into it overlaps its last value
        assert call(f=swapped(i, trace.data_ptr() + 39 * 8), tr=trace.data_ptr()) == (E, 0)
        for j in range(i):                                                          # any two of the seven overlapping
            assert call(f=swapped(i, seven[j])) == (E, 0)
            assert call(f=swapped(i, seven[j] + n_bytes - 8)) == (E, 0)             # ... by one cell
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


def test_cg_solve_is_unchanged(nh):
    """cg_solve on cg_cases' problem gives, after BiCGStab has run in this process (and has grown and used the device block
    the solvers share), the bits it gave before the first BiCGStab call"""
    P = _problem(nh, "f64_12x20x136")
    _solve(nh, P, 5, 0.0, check_every=5)
    assert nh.apply.cg_counts() == (5, 0, 1)
    (res1, x1, r1, p1), (res2, x2, r2, p2) = nh.cg_before, _cg_run(nh)
    assert nh.apply.cg_counts() == (10, 0, 1)
    assert res1[:3] == res2[:3] and bits_equal(res1[3], res2[3])
    assert bits_equal(x1, x2) and bits_equal(r1, r2) and bits_equal(p1, p2)
    assert res1[2] < 1e-8 * res1[1]
