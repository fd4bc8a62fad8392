"""neptune_hip_pcg_solve: conjugate gradients with a Jacobi preconditioner fused into the solver's kernels.

Operator: pcg_cases.pcg_module -- (d + w) * centre - (star neighbours), d = 12, w a coefficient field (input 1) drawn per cell
from {0, 16, 256, 4096}; minv = 1 / (d + w) on the interior, 1 on the rim.

Replay: the solver keeps a trace of its device scalars (pq_k, rz_(k+1), rr_(k+1)) and reports rz_0.  pcg_cases.replay runs the
recurrences of the definition in numpy with alpha_k and beta_k formed from THOSE scalars (one division each, in the element
type), z = minv * r rounded once, and q from the oracle's operator; whatever order the device summed in, x, r and p must then
agree bit for bit, and each traced scalar must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the replay's own terms.

Stop: thresholds sit at the geometric mean of two consecutive check values of a numpy run of the same recurrences, which
differ by a factor of 2 at least (tests/test_pcg_host.py pins a factor of 2 per iteration over these iterations), so the
threshold is a factor sqrt(2) away from both and the iteration count follows from the definition as long as the device's r . r
is within that factor of numpy's -- which the test asserts."""
import ctypes as C
import math

import numpy as np
import pytest

import cg_cases as cc
import helpers
import pcg_cases as pc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

# name: (shape, dtype, non-zero rim values in x)
PROBLEMS = {
    "f64_12x20x136": ((12, 20, 136), np.float64, False),
    "f32_12x20x136": ((12, 20, 136), np.float32, False),
    "f64_9x11x131_rim": ((9, 11, 131), np.float64, True),     # n = 12969 is odd: the vector kernels' tail runs
    "f32_9x11x131": ((9, 11, 131), np.float32, False),        # n % 4 == 1: their f32 tail
    "f64_8x512x520": ((8, 512, 520), np.float64, False),         # 2 129 920 cells: past the 2 097 152 lanes of the capped grid
}
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
    ns.cache, ns.keep = {}, []
    return ns


def _problem(nh, name):
    """the compiled operator, its oracle, w / x0 / b / minv and the numpy run's r . r sequence: computed once per problem, left
    unchanged"""
    if name not in nh.cache:
        shape, dtype, rim = PROBLEMS[name]
        P = pc.Problem(shape, dtype, rim=rim)
        P.entry = nh.lowering.compile_module(P.text, dot_entries=True).dot_entry("entry")
        P.seq = pc.numpy_pcg(P.A, P.x0, P.b, P.minv, P.where, pc.STOP_ITERS[dtype]) if name != BIG else None
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


def _solve(nh, P, max_iters, tol2, check_every=1, trace=False, dot="auto", x0=None, b=None, minv=None, offset=0, fields=None):
    """-> (result of cg_solve, x, [r, p, q] as numpy, the device fields used).  The work fields are pre-filled with NaN: the
    solver must not depend on what they hold.  fields: the (x, b, work, w) of an earlier call, used again."""
    F = nh.fields.DeviceField
    make = (lambda a: _offset_field(nh, a, offset)) if offset else F.from_numpy
    nan = np.full(P.shape, np.nan, P.dtype)
    if fields is None:
        x, bf, work, w = make(P.x0 if x0 is None else x0), make(P.b if b is None else b), [make(nan) for _ in range(3)], F.from_numpy(P.w)
    else:
        x, bf, work, w = fields
        x.tensor.copy_(nh.torch.from_numpy(np.ascontiguousarray(P.x0 if x0 is None else x0)))
        for f in work:
            f.tensor.fill_(float("nan"))
    m = F.from_numpy(P.minv if minv is None else minv)
    nh.keep.append(m)     # every preconditioner of this module stays allocated: two of them never share an address
    res = nh.apply.cg_solve(P.entry, x, bf, P.bounds, max_iters, tol2, check_every=check_every, others=[w], trace=trace, dot=dot,
                            work=work, minv=m)
    nh.torch.cuda.synchronize()
    return res, x.numpy(), [f.numpy() for f in work], (x, bf, work, w)


def _check_replay(nh, name, iters, check_every, dot="auto", path="fused", minv=None, offset=0, fields=None, solves=True):
    P = _problem(nh, name)
    minv = P.minv if minv is None else minv
    (done, rr0, rr_last, trace), x, (r, p, q), used = _solve(nh, P, iters, 0.0, check_every=check_every, trace=True, dot=dot,
                                                            minv=minv, offset=offset, fields=fields)
    rz0 = nh.apply.pcg_rz0()
    fused, fallback, checks = nh.apply.cg_counts()
    assert done == iters and trace.shape == (iters, 3)
    assert checks == -(-iters // check_every)
    assert (fused, fallback) == ((iters, 0) if path == "fused" else (0, iters))
    _, _, (rz0_ref, rz0_bound), (rr0_ref, rr0_bound) = pc.setup(P.A, P.x0, P.b, minv, P.where)
    print(f"{name} {path}: rz0 = {rz0!r} (terms' sum {rz0_ref!r}, bound {rz0_bound:.3e})  rr0 = {rr0!r} (sum {rr0_ref!r}, "
          f"bound {rr0_bound:.3e})")
    assert abs(rz0 - rz0_ref) <= rz0_bound and abs(rr0 - rr0_ref) <= rr0_bound
    xr, rr_, pr, refs = pc.replay(P.A, P.x0, P.b, minv, P.where, rz0, trace)
    for k, sums in enumerate(refs):
        print(f"  k={k}: " + "  ".join(f"{nm} = {trace[k][c]!r} (sum {s!r}, bound {bd:.3e})"
                                        for c, (nm, (s, bd)) in enumerate(zip(("pq", "rz'", "rr'"), sums))))
        for c, (s, bd) in enumerate(sums):
            assert abs(float(trace[k][c]) - s) <= bd
    assert rr_last == float(trace[-1][2])
    assert bits_equal(x, xr), mismatch_report(x, xr)
    assert bits_equal(r, rr_), mismatch_report(r, rr_)
    assert bits_equal(p, pr), mismatch_report(p, pr)
    # cells of x outside Omega are never written; r and p are +0 there
    outside = np.ones(P.shape, bool)
    outside[P.where] = False
    assert bits_equal(x[outside], P.x0[outside])
    zero = np.zeros(int(outside.sum()), P.dtype)
    assert bits_equal(r[outside], zero) and bits_equal(p[outside], zero)
    # ... and it is a solve: r . r has fallen by 2x per iteration at least (the numpy run's does: test_pcg_host.py)
    if solves:
        assert rr_last <= rr0 / 2.0 ** iters
    return used, x, trace, rz0


@pytest.mark.parametrize("name,iters", [("f64_12x20x136", 8), ("f32_12x20x136", 6), ("f64_9x11x131_rim", 8), ("f32_9x11x131", 6)])
def test_replay_from_the_traced_scalars_reproduces_every_vector(nh, name, iters):
    _check_replay(nh, name, iters, check_every=1)


def test_more_cells_than_lanes_take_the_grid_stride_loops_round_again(nh):
    """2 129 920 cells in fields one element off 16-byte alignment: the scalar forms' grid is capped at 256 * 32 workgroups
    (2 097 152 lanes), so 32 768 lanes make a second trip.  Two iterations: a wrong stride, or a cell summed twice, shows in
    the vectors, in rz' and in rr'.  (The fall of r . r per iteration is pinned on the small problems only.)"""
    _check_replay(nh, BIG, 2, check_every=2, offset=1, solves=False)


def test_fields_at_an_8_byte_offset_run_the_scalar_kernel_forms(nh):
    """x, b, r, p, q one f64 element into larger allocations: not 16-byte aligned, so the grid-stride forms of the update and
    direction kernels run"""
    _check_replay(nh, "f64_9x11x131_rim", 8, check_every=3, offset=1)


def test_a_block_replayed_as_a_graph_and_again_with_another_preconditioner(nh):
    """one block of 10 iterations: the first one plain, eight from a captured graph, one plain.  Then the same call on the same
    fields with another minv: a graph captured with one preconditioner must not be replayed with another."""
    name = "f64_12x20x136"
    P = _problem(nh, name)
    used, x1, _, _ = _check_replay(nh, name, 10, check_every=10)
    other = np.ones(P.shape, P.dtype)
    other[P.where] = (2.0 * P.minv[P.where] + 0.25).astype(P.dtype)      # positive, another preconditioner altogether
    _, x2, _, _ = _check_replay(nh, name, 10, check_every=10, minv=other, fields=used, solves=False)
    assert not bits_equal(x1, x2)
    # and back: the first preconditioner's graph is still the first preconditioner's
    _, x3, _, _ = _check_replay(nh, name, 10, check_every=10, fields=used)
    assert bits_equal(x1, x3)


@pytest.mark.parametrize("name,stop_check", [("f64_12x20x136", 3), ("f32_12x20x136", 2)])
@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("dot", ["auto", "fallback"])
def test_stops_where_the_definition_stops(nh, name, stop_check, check_every, dot):
    P = _problem(nh, name)
    max_iters = pc.STOP_ITERS[P.dtype]
    # between the check values number stop_check - 1 and stop_check
    tol2 = cc.tol_between(P.seq, (stop_check - 1) * check_every, stop_check * check_every)
    want_done, want_checks = cc.expected_stop(P.seq, check_every, max_iters, tol2)
    assert want_done == stop_check * check_every and want_checks == stop_check
    (done, rr0, rr_last), _, _, _ = _solve(nh, P, max_iters, tol2, check_every=check_every, dot=dot)
    fused, fallback, checks = nh.apply.cg_counts()
    print(f"{name} check_every={check_every} {dot}: iters={done} rr0={rr0!r} rr_last={rr_last!r} numpy {P.seq[done]!r} tol2={tol2!r}")
    assert done == want_done and checks == want_checks
    assert (fused, fallback) == ((done, 0) if dot == "auto" else (0, done))
    assert rr_last <= tol2
    # what the threshold's place relies on: the device's r . r within sqrt(2) of the numpy run's
    assert P.seq[done] / math.sqrt(2.0) <= rr_last <= P.seq[done] * math.sqrt(2.0)


def test_fallback_runs_the_same_iteration(nh):
    _check_replay(nh, "f64_9x11x131_rim", 8, check_every=3, dot="fallback", path="fallback")


def test_unit_preconditioner_is_plain_cg(nh):
    """minv = 1 everywhere: 1 * r is r, so rz and rr are sums of the same terms on the same tree, and the plain solver's
    definition (cg_cases.replay) fed this run's scalars reproduces x bit for bit: the two definitions coincide there"""
    name = "f64_9x11x131_rim"
    P = _problem(nh, name)
    ones = np.ones(P.shape, P.dtype)
    _, x, trace, rz0 = _check_replay(nh, name, 8, check_every=3, minv=ones, solves=False)
    assert bits_equal(np.ascontiguousarray(trace[:, 1]), np.ascontiguousarray(trace[:, 2]))
    xr, _, _, _ = cc.replay(P.A, P.x0, P.b, P.where, rz0, [(row[0], row[1]) for row in trace])
    assert bits_equal(x, xr), mismatch_report(x, xr)


def test_exact_breakdown_leaves_everything_as_it_is(nh):
    P = _problem(nh, "f64_9x11x131_rim")
    b = P.A(P.x0)                      # b = A(x) exactly: the residual is +0 everywhere on Omega
    (done, rr0, rr_last), x, _, _ = _solve(nh, P, 5, 0.0, b=b)
    assert (done, rr0, rr_last) == (0, 0.0, 0.0) and nh.apply.pcg_rz0() == 0.0 and nh.apply.cg_counts() == (0, 0, 0)
    assert bits_equal(x, P.x0)
    # tol2 < 0 forces the iterations to run: alpha = beta = 0, nothing moves, nothing becomes NaN
    (done, rr0, rr_last, trace), x, (r, p, q), _ = _solve(nh, P, 3, -1.0, trace=True, b=b)
    assert (done, rr0, rr_last) == (3, 0.0, 0.0) and nh.apply.cg_counts() == (3, 0, 3)
    assert bits_equal(x, P.x0)
    zero = np.zeros(P.shape, P.dtype)
    assert bits_equal(r, zero) and bits_equal(p, zero) and np.isfinite(q).all()
    assert bits_equal(trace, np.zeros((3, 3), P.dtype))


def test_refusals_launch_nothing(nh):
    P = _problem(nh, "f64_12x20x136")
    F = nh.fields.DeviceField
    x, b, w, m = F.from_numpy(P.x0), F.from_numpy(P.b), F.from_numpy(P.w), F.from_numpy(P.minv)
    work = [F.empty_like(x) for _ in range(3)]
    x.tensor.fill_(-3.0)
    for f in work:
        f.tensor.fill_(-5.0)
    g = nh.apply.geom_for([x, w], work[2], P.bounds)
    n_bytes = x.tensor.numel() * 8
    trace = nh.torch.full((3 * 8 + 16,), -7.0, dtype=nh.torch.float64, device="cuda")
    st = nh.fields.current_stream_ptr()
    rest = (C.c_void_p * 1)(w.ptr)

    def call(mp=m.ptr, tr=None, max_iters=8, check_every=1):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = nh.lib.neptune_hip_pcg_solve(C.cast(P.entry.fn, C.c_void_p), C.cast(P.entry.fn_dot, C.c_void_p), -1, x.dtype, C.byref(g),
                                          x.ptr, b.ptr, mp, (C.c_void_p * 3)(*[f.ptr for f in work]), rest, max_iters, check_every,
                                          1e-30, tr, st, None, C.byref(done), C.byref(rr0), C.byref(last))
        return rc, done.value
    E = nh.capi.EINVAL
    assert call(mp=None) == (E, 0)                                                  # a null minv
    assert call(mp=m.ptr + 4) == (E, 0)                                             # misaligned for f64
    for f in [x, b] + work:
        assert call(mp=f.ptr) == (E, 0)                                             # minv is one of the five fields
        assert call(mp=f.ptr + n_bytes - 8) == (E, 0)                               # ... or starts in its last cell
    assert call(tr=m.ptr + 16) == (E, 0)                                            # a trace inside minv
    assert call(tr=work[1].ptr + 16) == (E, 0)                                      # a trace inside p
    # the trace is 3 * max_iters values long: used as minv, a field that starts 20 values into it overlaps (2 * 8 would not)
    assert call(mp=trace.data_ptr() + 20 * 8, tr=trace.data_ptr()) == (E, 0)
    assert call(check_every=0) == (E, 0) and call(max_iters=-1) == (E, 0)           # the plain solver's refusals
    nh.torch.cuda.synchronize()
    assert bool((x.tensor == -3.0).all()) and all(bool((f.tensor == -5.0).all()) for f in work)
    assert bool((trace == -7.0).all()) and bits_equal(b.numpy(), P.b) and bits_equal(m.numpy(), P.minv)


@pytest.mark.parametrize("name", ["f64_9x11x131_rim", "f32_12x20x136"])
def test_operator_diagonal_is_the_oracles_probing_and_the_exact_diagonal(nh, name):
    P = _problem(nh, name)
    F = nh.fields.DeviceField
    like, w = F.from_numpy(P.x0), F.from_numpy(P.w)
    got = nh.apply.operator_diagonal(P.entry, like, P.bounds, others=[w]).numpy()
    assert P.entry.halo0 == 1
    want = pc.probe_diagonal(P.A, P.shape, P.dtype, P.where, reach=1)
    assert bits_equal(got, want), mismatch_report(got, want)
    assert bits_equal(got, P.diag) and bits_equal(got[P.where], (P.dtype(12) + P.w[P.where]).astype(P.dtype))
    minv = nh.apply.jacobi_minv(P.entry, like, P.bounds, others=[w]).numpy()
    assert bits_equal(minv, P.minv), mismatch_report(minv, P.minv)


def test_jacobi_minv_raises_on_a_zero_diagonal(nh):
    P = _problem(nh, "f64_9x11x131_rim")
    F = nh.fields.DeviceField
    w0 = pc.w_field(P.shape, P.dtype, values=(-12.0, 16.0, 256.0, 4096.0))       # d + w = 0 on a quarter of the cells
    assert (w0[P.where] == -12.0).any()
    like, w = F.from_numpy(P.x0), F.from_numpy(w0)
    diag = nh.apply.operator_diagonal(P.entry, like, P.bounds, others=[w]).numpy()
    assert bits_equal(diag, pc.diagonal(w0, P.where))
    with pytest.raises(ValueError, match="0 or not finite"):
        nh.apply.jacobi_minv(P.entry, like, P.bounds, others=[w])
    # a zero outside Omega does not matter: the rim of w is never the diagonal's business
    w1 = P.w.copy()
    w1[0] = -12.0
    assert bits_equal(nh.apply.jacobi_minv(P.entry, like, P.bounds, others=[F.from_numpy(w1)]).numpy(), P.minv)


def test_operator_diagonal_refuses_a_reach_the_operator_exceeds(nh):
    """a radius-2 star probed with reach 1: cells of one colour would see each other, so the guard launch refuses; with the
    entry's own halo0 = 2 the diagonal is the centre weight"""
    shape = (9, 11, 131)
    entry = nh.lowering.compile_module(cc.cg_module(shape, radius=2)).geom_entry("entry")
    like = nh.fields.DeviceField.from_numpy(np.zeros(shape))
    bounds = cc.interior(shape, 2)
    with pytest.raises(ValueError, match="reaches further"):
        nh.apply.operator_diagonal(entry, like, bounds, reach=1)
    assert entry.halo0 == 2
    want = np.zeros(shape)
    want[tuple(slice(2, n - 2) for n in shape)] = 24.0
    got = nh.apply.operator_diagonal(entry, like, bounds).numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
