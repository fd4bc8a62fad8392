"""neptune_hip_mgcg_solve: conjugate gradients preconditioned with one V-cycle, whose fields never leave the
device, against the NumPy restatement of tests/mg_restatement.py.

The restatement's recurrences driven by the DEVICE's traced scalars (rz_0 and the rows pq_k, rz_(k+1), rr_(k+1)) must
reproduce x, r, p, z and every level's x_l, b_l bit for bit, whatever the launch path (plain launches or the replayed graph
of one iteration; the dot-monitored launch or the fallback).  Every traced scalar, rr_0 and rz_0 must lie within
2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms.

Operator: mg_cases.mg_module, the unscaled Poisson star, one lowered module per level shape, rscale = 4; minv_0 =
omega / (2 rank) on Omega and +0 outside (the definition forms z = minv_0 * r on the whole box), the coarser minv NaN outside
Omega; the work fields r, p, z, q_l and x_l, b_l (l >= 1) hold NaN before every call.

Stop: thresholds sit at the geometric mean of two consecutive check values of the restatement's r . r sequence, which the
test first requires to differ by a factor of 4 (tests/test_mgcg_host.py pins that the sequence falls that fast)."""
import ctypes as C

import numpy as np
import pytest

import cg_cases
import helpers
import mg_cases as mgc
import mg_device as mgd
import mg_restatement as rst
import mgcg_cases as mg
import pcg_cases as pc
from helpers import bits_equal

pytestmark = pytest.mark.gpu

# name: (Omega of level 0, levels, omega, dtype)
PROBLEMS = {
    "3d_f64": ((7, 15, 263), 3, 6.0 / 7.0, np.float64),
    "3d_f32": ((7, 15, 263), 3, 6.0 / 7.0, np.float32),
    "2d_f64": ((15, 263), 3, 0.8, np.float64),
}
PCG_OMEGA = (7, 15, 31)      # the two-input operator: two levels, 9 x 17 x 33 -> 5 x 9 x 17
BUILTIN_OMEGA = (7, 15, 31)
# more cells than one round of the capped flat grid (256 * 32 workgroups of 256 lanes): the box of
# tests/test_pcg_solve_gpu.py's largest problem, 8 x 512 x 520 = 2 129 920 cells, with Omega 5 x 509 x 517 at (1, 1, 1)
BIG_RIMS = [([1, 1, 1], [2, 2, 2]), ([1, 1, 1], [1, 1, 1])]
BIG_OMEGA = (5, 509, 517)


def _texts():
    out = {}
    for name, (omega, n_levels, _, dtype) in PROBLEMS.items():
        out[name] = [mgc.mg_module(shape, dtype) for shape, _ in mgc.level_shapes(omega, n_levels)]
    out["pcg"] = [pc.pcg_module(shape, np.float64) for shape, _ in mgc.level_shapes(PCG_OMEGA, 2)]
    out["builtin"] = [mgc.mg_module(shape, np.float64) for shape, _ in mgc.level_shapes(BUILTIN_OMEGA, 2)][1:]
    out["big"] = [mgc.mc.star_module(shape, np.float64, bounds=([s.start for s in where], [s.stop for s in where]), centre=6.0, side=-1.0)
                  for shape, where in mgc.level_shapes(BIG_OMEGA, 2, BIG_RIMS)]
    return out


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.texts = _texts()
    # every module once, side by side: level 0's with their dot entries ("builtin" lists level 1 alone)
    mgd.prefetch([(t, l == 0 and name != "builtin") for name, ts in ns.texts.items() for l, t in enumerate(ts)])
    return ns


def _fields(P, rim=False):
    P.x0, P.b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype, rim=rim)


def _problem(nh, name, rim=False):
    def build(P):
        omega, n_levels, damp, P.dtype = PROBLEMS[name]
        P.ref, P.texts = mg.star_levels(omega, n_levels, P.dtype, damp, texts=nh.texts[name])
        _fields(P, rim)
    return mgd.problem(nh, (name, rim), build, dots=(0,))


def _check_replay(nh, P, iters, **kw):
    """mg_device.check_replay, and what the fields hold outside Omega"""
    return mgd.check_replay(nh, P, iters, outside=True, **kw)


@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    P = _problem(nh, name)
    R = _check_replay(nh, P, iters, want_counts=(2, 0, 0, 2) if iters == 2 else (1, 4, 0, 5))
    # ... and it is a solve: r . r falls by 4x per iteration at least (the restatement's does: test_mgcg_host.py)
    assert R.res[2] <= R.res[1] / 4.0 ** iters


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    P = _problem(nh, "3d_f64")
    monkeypatch.delenv("NEPTUNE_HIP_MG_GRAPH", raising=False)
    G = mgd.cg(nh, P, 5)
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "0")          # read at every call
    Pl = _check_replay(nh, P, 5, want_counts=(5, 0, 0, 5))
    assert G.counts == (1, 4, 0, 5)
    mgd.same_runs(G, Pl)


def test_fallback_runs_the_same_iteration(nh):
    """dot = "fallback": a plain launch and neptune_hip_dot: another summation order for pq.  Each run's scalars lie within
    the bounds of its own terms' exact sums and its fields replay from its own trace; the set-up is the same, bit for bit, so
    both runs' pq_0 are sums of the same terms and differ by at most twice the bound"""
    P = _problem(nh, "3d_f64")
    A = _check_replay(nh, P, 5, check_every=2, want_counts=(1, 4, 0, 3))
    F = _check_replay(nh, P, 5, check_every=2, dot="fallback", want_counts=(1, 4, 5, 3))
    assert F.res[1] == A.res[1] and F.rz0 == A.rz0      # the set-up does not depend on the dot entry
    assert abs(float(F.res[3][0][0]) - float(A.res[3][0][0])) <= 2.0 * A.checks[0][0][1]


@pytest.mark.parametrize("name,check_every,between", [("3d_f64", 1, (2, 3)), ("3d_f64", 3, (3, 6)), ("2d_f64", 3, (3, 6)),
                                                      ("3d_f32", 1, (1, 2))])
def test_stops_where_the_definition_says(nh, name, check_every, between):
    P = _problem(nh, name)
    sequence = lambda: rst.numpy_mgcg(P.ref, P.x0, P.b, 6 if P.dtype == np.float64 else 3)
    seq, tol2, max_iters, want = mgd.stop_schedule(P, sequence, check_every, between)
    R = mgd.cg(nh, P, max_iters, tol2=tol2, check_every=check_every, trace=False)
    mgd.check_cg_stop(R, seq, tol2, want, label=f"{name}: ")


def test_a_converged_start_runs_no_iteration(nh):
    P = _problem(nh, "3d_f64")
    rr0_ref = cg_cases.dot_terms(P.b, P.b, P.ref[0].where)          # x0 = 0: r = b on Omega
    R = mgd.cg(nh, P, 5, tol2=2.0 * rr0_ref[0])
    done, rr0, rr_last, trace = R.res
    assert (done, R.counts, R.rz0, trace.shape) == (0, (0, 0, 0, 0), 0.0, (0, 3))
    assert rr0 == rr_last and abs(rr0 - rr0_ref[0]) <= rr0_ref[1]
    assert bits_equal(R.x, P.x0) and bits_equal(R.b, P.b)
    # max_iters = 0: rr_0 is still formed
    R = mgd.cg(nh, P, 0, trace=False)
    assert R.res == (0, rr0, rr0) and R.counts == (0, 0, 0, 0) and bits_equal(R.x, P.x0)


def test_fields_at_an_8_byte_offset_run_the_scalar_kernel_forms(nh):
    """x, b, r, p, z, q_0 and minv_0 one f64 element into larger allocations: not 16-byte aligned, so the grid-stride forms of
    the update and direction kernels run"""
    _check_replay(nh, _problem(nh, "3d_f64"), 3, check_every=2, offset=8, want_counts=(1, 2, 0, 2))


def test_more_cells_than_lanes_take_the_grid_stride_loops_round_again(nh):
    """2 129 920 cells in fields one element off 16-byte alignment: the scalar forms' grid is capped at 256 * 32 workgroups
    (2 097 152 lanes), so 32 768 lanes make a second trip; unequal rims on level 0.  Two iterations of V(1, 1) with two coarse
    sweeps: a wrong stride, or a cell summed twice, shows in the fields, in rz' and in rr'."""
    def build(P):
        P.dtype, P.texts = np.float64, nh.texts["big"]
        shapes = mgc.level_shapes(BIG_OMEGA, 2, BIG_RIMS)
        P.ref = [rst.Level(rst.Operator(text), shape, where, mgc.minv_field(shape, where, np.float64, 6.0 / 7.0, outside=0.0 if l == 0 else np.nan),
                           np.float64) for l, (text, (shape, where)) in enumerate(zip(P.texts, shapes))]
        _fields(P)
    P = mgd.problem(nh, "big", build, dots=(0,))
    _check_replay(nh, P, 2, check_every=2, offset=8, sweeps=1, coarse_sweeps=2, want_counts=(2, 0, 0, 1))


def test_nonzero_dirichlet_rim(nh):
    P = _problem(nh, "3d_f64", rim=True)
    R = _check_replay(nh, P, 2)
    outside = np.ones(P.x0.shape, bool)
    outside[P.ref[0].where] = False
    assert np.count_nonzero(P.x0[outside]) > 0 and bits_equal(R.x[outside], P.x0[outside])
    zero = mgd.cg(nh, _problem(nh, "3d_f64"), 2)
    assert not bits_equal(R.x, zero.x)        # the rim values did enter, through A(x)


def test_two_input_operator_with_a_coefficient_per_level(nh):
    """pcg_cases.pcg_module on two levels, w injected to the coarse grid in numpy: in_rest per level"""
    def build(P):
        dtype = P.dtype = np.float64
        shapes = mgc.level_shapes(PCG_OMEGA, 2)
        P.texts = nh.texts["pcg"]
        w = [pc.w_field(shapes[0][0], dtype, values=(0.0, 1.0, 2.0, 4.0))]
        wc = np.zeros(shapes[1][0], dtype)
        wc[shapes[1][1]] = w[0][shapes[0][1]][1::2, 1::2, 1::2]     # the coarse cell j sits on the fine cell 2 j + 1
        w.append(wc)
        P.ref = []
        for l, (text, (shape, where), wl) in enumerate(zip(P.texts, shapes, w)):
            minv = np.full(shape, 0.0 if l == 0 else np.nan, dtype)
            minv[where] = (dtype(0.8) / (dtype(12.0) + wl[where])).astype(dtype)     # pcg_module's diagonal is 4 rank + w
            P.ref.append(rst.Level(rst.Operator(text, wl), shape, where, minv, dtype))
        P.rests = [[nh.fields.DeviceField.from_numpy(wl)] for wl in w]
        _fields(P)
    P = mgd.problem(nh, "pcg", build, dots=(0,))
    R = _check_replay(nh, P, 3, want_counts=(1, 2, 0, 3))
    assert R.res[2] < R.res[1]


def test_builtin_body_on_level_zero(nh):
    """level 0 runs the built-in 7-point body (fn = NULL: its dot-monitored launch is neptune_hip_apply_builtin_dot), level 1
    a lowered module"""
    dtype = np.float64
    shapes = mgc.level_shapes(BUILTIN_OMEGA, 2)
    P = mgd.Problem()
    P.dtype = dtype
    A0 = lambda u: helpers.oracle_entry("3d7", u)
    P.ref = [rst.Level(A0, shapes[0][0], shapes[0][1], mgc.minv_field(shapes[0][0], shapes[0][1], dtype, 0.125, outside=0.0), dtype),
             rst.Level(rst.Operator(nh.texts["builtin"][0]), shapes[1][0], shapes[1][1],
                       mgc.minv_field(shapes[1][0], shapes[1][1], dtype, 0.8), dtype)]
    P.entries = [nh.capi.BODY_LAP3D7_F64, mgd.entry(nh, nh.texts["builtin"][0])]
    P.x0, P.b = mgc.problem_fields(shapes[0][0], shapes[0][1], dtype)
    _check_replay(nh, mgd.finish(nh, P), 3, want_counts=(1, 2, 0, 3))


def test_exact_breakdown_leaves_everything_as_it_is(nh):
    P = _problem(nh, "3d_f64", rim=True)
    b = P.ref[0].A(P.x0)                      # b = A(x) exactly: the residual is +0 everywhere on Omega
    R = mgd.cg(nh, P, 5, b=b)
    assert R.res[:3] == (0, 0.0, 0.0) and R.rz0 == 0.0 and R.counts == (0, 0, 0, 0)
    assert bits_equal(R.x, P.x0)
    # tol2 < 0 forces the iterations to run: alpha = beta = 0, nothing moves, nothing becomes NaN
    R = mgd.cg(nh, P, 3, tol2=-1.0, b=b)
    done, rr0, rr_last, trace = R.res
    assert (done, rr0, rr_last) == (3, 0.0, 0.0) and R.rz0 == 0.0 and R.counts[0] + R.counts[1] == 3 and R.counts[3] == 3
    assert bits_equal(R.x, P.x0)
    zero = np.zeros(P.x0.shape, P.dtype)
    for a in (R.r, R.p, R.z):
        assert bits_equal(a, zero)
    assert np.isfinite(R.q[0]).all() and bits_equal(trace, np.zeros((3, 3), P.dtype))


def test_python_wrapper(nh):
    P = _problem(nh, "3d_f64")
    h, x, b, _ = mgd.hierarchy(nh, P)
    ref = mgd.cg(nh, P, 4)
    # its defaults: V(2, 2), 8 coarse sweeps, no trace, work fields of its own, the entry's own dot entry
    res = nh.mg.cg_solve(h, x, b, max_iters=4)
    assert len(res) == 3 and res == ref.res[:3] and bits_equal(x.numpy(), ref.x)
    assert nh.mg.cg_counts() == (1, 3, 0, 4) and nh.mg.cg_rz0() == ref.rz0
    with pytest.raises(ValueError, match="dot is"):
        nh.mg.cg_solve(h, x, b, dot="never")
    with pytest.raises(ValueError, match="two levels"):
        nh.mg.cg_solve(nh.mg.Hierarchy(h.levels[:1]), x, b)
    with pytest.raises(ValueError, match="box"):
        nh.mg.cg_solve(h, h.q[1], b)


def test_refusals_on_device_pointers(nh):
    P = _problem(nh, "3d_f64")
    h, x, b, work = mgd.hierarchy(nh, P)
    E, lib = nh.capi.EINVAL, nh.lib
    x.tensor.fill_(-3.0)
    for f in work:
        f.tensor.fill_(-5.0)
    trace = nh.torch.full((3 * 4 + 16,), -7.0, dtype=nh.torch.float64, device="cuda")
    n_bytes = int(np.prod(P.ref[0].shape)) * 8

    def call(change=None, n_levels=3, dtype=nh.capi.F64, sweeps=2, coarse=8, max_iters=4, check_every=1, stream=None, w=None, tr=None):
        arr, keep = h._structs(x, b)
        if change:
            change(arr)
        ptrs = [f.ptr for f in work] if w is None else w
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        st = nh.fields.current_stream_ptr() if stream is None else stream
        rc = lib.neptune_hip_mgcg_solve(arr, n_levels, dtype, None, sweeps, coarse, (C.c_void_p * 3)(*ptrs), max_iters, check_every, 0.0,
                                        tr, st, None, C.byref(done), C.byref(rr0), C.byref(last))
        return rc, done.value, rr0.value, last.value

    R = (E, 0, 0.0, 0.0)
    assert call(n_levels=1) == R and call(n_levels=0) == R and call(n_levels=17) == R and call(dtype=5) == R
    assert call(sweeps=0) == R and call(sweeps=-1) == R and call(coarse=-1) == R
    assert call(check_every=0) == R and call(max_iters=-1) == R
    wp = [f.ptr for f in work]
    for i in range(3):
        assert call(w=wp[:i] + [None] + wp[i + 1:]) == R and call(w=wp[:i] + [wp[i] + 4] + wp[i + 1:]) == R
        for o in range(3):
            if o != i:
                assert call(w=wp[:i] + [wp[o] + n_bytes - 8] + wp[i + 1:]) == R, (i, o)
        for level in (0, 1):
            for field in ("x", "b", "q", "minv"):
                assert call(lambda a: setattr(a[level], field, wp[i] + 8)) == R, (i, level, field)
                assert call(w=wp[:i] + [getattr(h._structs(x, b)[0][level], field)] + wp[i + 1:]) == R, (i, level, field)
        assert call(tr=wp[i] + 16) == R
    for level in (0, 1):
        for field in ("x", "b", "q", "minv"):
            assert call(tr=getattr(h._structs(x, b)[0][level], field) + 8) == R, (level, field)
    # the trace is 3 * max_iters = 12 values long: a field that starts 10 values into it overlaps
    assert call(w=[wp[0], trace.data_ptr() + 80, wp[2]], tr=trace.data_ptr()) == R
    assert call(tr=trace.data_ptr() + 4) == R
    # those of neptune_hip_mg_solve
    for field in ("x", "b", "q", "minv"):
        for level in range(3):
            assert call(lambda a: setattr(a[level], field, None)) == R, (field, level)
            for other in ("x", "b", "q", "minv"):
                if other != field:
                    assert call(lambda a: setattr(a[level], field, getattr(a[level], other))) == R, (field, other, level)
        assert call(lambda a: setattr(a[2], field, a[1].b + 8)) == R

    def other_rank(a):
        a[2].g.rank = 2
    assert call(other_rank) == R

    def smaller_omega(a):
        a[1].g.ub[2] -= 1
    assert call(smaller_omega) == R

    def empty(a):
        a[0].g.region_ub[0] = a[0].g.region_lb[0]
    assert call(empty) == R
    assert call(lambda a: setattr(a[0], "rscale", float("nan"))) == R
    # a call while the stream is being captured: rr could not be read back
    torch = nh.torch
    side = torch.cuda.Stream()
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        scratch.add_(1.0)
        captured = call(stream=int(side.cuda_stream))
    assert captured == R
    torch.cuda.synchronize()
    assert bool((x.tensor == -3.0).all()) and bits_equal(b.numpy(), P.b) and bool((trace == -7.0).all())
    assert all(bool((f.tensor == -5.0).all()) for f in work)
    assert all(bool(nh.torch.isnan(f.tensor).all()) for f in h.q + h.x[1:] + h.b[1:])
    assert nh.mg.cg_counts() == (0, 0, 0, 0) and nh.mg.cg_rz0() == 0.0
