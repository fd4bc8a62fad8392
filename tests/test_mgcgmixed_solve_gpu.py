"""neptune_hip_mgcg_solve_mixed: conjugate gradients in f64 around a V-cycle in f32, whose fields never leave
the device, against the NumPy restatement of tests/mg_restatement.py.

The restatement's recurrences driven by the DEVICE's traced scalars (rz_0 and the rows pq_k, rz_(k+1), rr_(k+1)) must
reproduce x, r, p in f64 and r32, z32 and every level's x_l, b_l in f32 bit for bit, whatever the launch path (plain launches
or the replayed graph of one iteration; the dot-monitored launch or the fallback; the 16-byte kernel forms, their tails, or
the grid-stride forms).  Every traced scalar, rr_0 and rz_0 must lie within 2 (n - 1) eps64 sum |t_i| of the exact sum of the
restatement's own f64 terms.

Operator: mg_cases.mg_module, the unscaled Poisson star, lowered at f64 for the outer operator and at f32 once per level
shape, rscale = 4; minv_0 = omega / (2 rank) on Omega and +0 outside, the coarser minv NaN outside Omega; every work field
holds NaN before a call.

Stop: thresholds sit at the geometric mean of two consecutive check values of the restatement's r . r sequence, which the
test first requires to differ by a factor of 4."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_device as mgd
import mg_restatement as rst
import mgcg_cases as mg
import mgcgmixed_cases as mx
import mglines_cases as lc
import mgsemi_cases as sc
import pcg_cases as pc
from helpers import bits_equal

pytestmark = pytest.mark.gpu

D, S = np.float64, np.float32
# name: (Omega of level 0, levels, omega, per-level rims or None).  Cells of level 0's box: 17^3 = 4913 = 4 k + 1;
# 33 x 33 = 1089 = 4 k + 1; 33 x 34 = 1122 = 4 k + 2; 33 x 35 = 1155 = 4 k + 3: the 16-byte forms' tails of 1, 2 and 3 cells
ONE = ([1, 1], [1, 1])
PROBLEMS = {
    "3d": ((15, 15, 15), 3, 6.0 / 7.0, None),
    "2d": ((31, 31), 3, 0.8, None),
    "2d_tail2": ((31, 31), 3, 0.8, [([1, 1], [1, 2]), ONE, ONE]),
    "2d_tail3": ((31, 31), 3, 0.8, [([1, 1], [1, 3]), ONE, ONE]),
}
PCG_OMEGA = (7, 15, 31)      # the two-input operator: two levels, 9 x 17 x 33 -> 5 x 9 x 17
BUILTIN_OMEGA = (7, 15, 31)
SEMI = ((15, 31), (1.0, 1.0), [(1,), (0, 1)])     # dim 0 kept on the first pair: 15 x 31 -> 15 x 15 -> 7 x 7
# more cells than one round of the capped flat grid (256 * 32 workgroups of 256 lanes): the box of
# tests/test_mgcg_solve_gpu.py's largest problem, 8 x 512 x 520 = 2 129 920 cells, with Omega 5 x 509 x 517 at (1, 1, 1)
BIG_RIMS = [([1, 1, 1], [2, 2, 2]), ([1, 1, 1], [1, 1, 1])]
BIG_OMEGA = (5, 509, 517)


def _star_text(shape, where, dtype):
    return mgc.mc.star_module(shape, dtype, bounds=([s.start for s in where], [s.stop for s in where]), centre=float(2 * len(shape)), side=-1.0)


def _star_texts(omega, n_levels, rims):
    """-> (level 0's f64 text, the f32 texts per level)"""
    shapes = mgc.level_shapes(omega, n_levels, rims)
    return _star_text(*shapes[0], D), [_star_text(shape, where, S) for shape, where in shapes]


def _texts():
    out = {name: _star_texts(omega, n_levels, rims) for name, (omega, n_levels, _, rims) in PROBLEMS.items()}
    shapes = mgc.level_shapes(PCG_OMEGA, 2)
    out["pcg"] = (pc.pcg_module(shapes[0][0], D), [pc.pcg_module(shape, S) for shape, _ in shapes])
    out["builtin"] = (None, [None, mgc.mg_module(mgc.level_shapes(BUILTIN_OMEGA, 2)[1][0], S)])
    out["big"] = _star_texts(BIG_OMEGA, 2, BIG_RIMS)
    steps = sc.with_axes(SEMI[0], SEMI[1], SEMI[2])
    out["semi"] = (mg.aniso_module(tuple(n + 2 for n in steps[0][0]), steps[0][1], D), sc.build_levels(steps, 0.8, S)[1])
    return out


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.texts = _texts()
    # every module once, side by side: the f64 ones with their dot entries (the outer operator's entry carries the
    # dot-monitored launch as well), the f32 ones plain
    jobs = [job for t64, t32 in ns.texts.values() for job in [(t64, True)] + [(t, False) for t in t32]]
    mgd.prefetch([(t, dot) for t, dot in jobs if t])
    return ns


class Case:
    """P: the restatement's Problem; entry64 / entries32; others64 / others32 (device fields); x0, b: left unchanged"""
    others64, others32 = (), None


def _finish(nh, T, texts, rim=False):
    if T.entry64 is None:
        T.entry64 = mgd.entry(nh, texts[0], True)
    T.entries32 = [e if e is not None else mgd.entry(nh, t, False) for e, t in zip(T.entries32, texts[1])]
    T.x0, T.b = mgc.problem_fields(T.P.shape, T.P.where, D, rim=rim)
    for a in (T.x0, T.b):
        a.setflags(write=False)
    T.runs = {}
    return T


def _star_levels(omega, n_levels, damp, rims, texts32):
    shapes = mgc.level_shapes(omega, n_levels, rims)
    return [rst.Level(rst.Operator(text), shape, where, mgc.minv_field(shape, where, S, damp, outside=0.0 if l == 0 else np.nan), S)
            for l, (text, (shape, where)) in enumerate(zip(texts32, shapes))]


def _case(nh, name, rim=False, stage_on_level_1=False):
    """the compiled operators and the restatement's problem: built once, x0 and b left unchanged"""
    key = (name, rim, stage_on_level_1)
    if key not in nh.cache:
        omega, n_levels, damp, rims = PROBLEMS[name]
        t64, t32 = nh.texts[name]
        T = Case()
        levels = _star_levels(omega, n_levels, damp, rims, t32)
        if stage_on_level_1:
            levels[1].stages = [lc.star_stage(levels[1], 1, damp)]
        T.P = mx.Problem(rst.Operator(t64), levels)
        T.entry64, T.entries32 = None, [None] * n_levels
        nh.cache[key] = _finish(nh, T, (t64, t32), rim)
    return nh.cache[key]


def _solve(nh, T, max_iters, tol2=0.0, check_every=1, trace=True, offset=0, b=None, **kw):
    """offset: in elements of each field's own type (mgcgmixed_cases.device_problem)"""
    dev = mx.device_problem(nh, T.P, T.entry64, T.entries32, T.x0, T.b if b is None else b, T.others64, T.others32, offset)
    res = nh.mg.cg_solve_mixed(dev.outer, dev.h, dev.x, dev.b, max_iters=max_iters, tol2=tol2, check_every=check_every, trace=trace,
                               work=dev.work, **kw)
    nh.torch.cuda.synchronize()
    return mgd.record(nh, res, dev.h, dev.x, dev.b, list(zip("rp", dev.work)) + [("r32", dev.h.b[0]), ("z32", dev.h.x[0])])


def _check_replay(nh, T, iters, check_every=1, want_counts=None, offset=0, **kw):
    """one traced run of `iters` iterations against the restatement's replay, and what the fields hold outside Omega; -> the run"""
    R = _solve(nh, T, iters, check_every=check_every, offset=offset, **kw)
    assert R.res[3].dtype == D
    sw = {k: v for k, v in kw.items() if k in ("sweeps", "coarse_sweeps")}
    mgd.compare_replay(R, T.P, T.x0, T.b, iters, check_every, want_counts, outside=True, **sw)
    return R


@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", ["2d", "3d"])
def test_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    T = _case(nh, name)
    R = _check_replay(nh, T, iters, want_counts=(2, 0, 0, 2) if iters == 2 else (1, 4, 0, 5))
    assert R.res[2] < R.res[1]


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    T = _case(nh, "3d")
    monkeypatch.delenv("NEPTUNE_HIP_MG_GRAPH", raising=False)
    G = _solve(nh, T, 5)
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "0")          # read at every call
    Pl = _check_replay(nh, T, 5, want_counts=(5, 0, 0, 5))
    assert G.counts == (1, 4, 0, 5)
    mgd.same_runs(G, Pl)


def test_fallback_runs_the_same_iteration(nh):
    """dot = "fallback": a plain launch and neptune_hip_dot: another summation order for pq.  Each run's scalars lie within
    the bounds of its own terms' exact sums and its fields replay from its own trace; the set-up is the same, bit for bit, so
    both runs' pq_0 are sums of the same terms and differ by at most twice the bound.  cg_counts() says which ran."""
    T = _case(nh, "3d")
    A = _check_replay(nh, T, 5, check_every=2, want_counts=(1, 4, 0, 3))
    F = _check_replay(nh, T, 5, check_every=2, dot="fallback", want_counts=(1, 4, 5, 3))
    assert F.res[1] == A.res[1] and F.rz0 == A.rz0      # the set-up does not depend on the dot entry
    assert abs(float(F.res[3][0][0]) - float(A.res[3][0][0])) <= 2.0 * A.checks[0][0][1]


@pytest.mark.parametrize("name,check_every,between", [("3d", 1, (2, 3)), ("3d", 3, (3, 6)), ("2d", 3, (3, 6))])
def test_stops_where_the_definition_says(nh, name, check_every, between):
    T = _case(nh, name)
    seq, tol2, max_iters, want = mgd.stop_schedule(T, lambda: rst.numpy_mgcg(T.P, T.x0, T.b, 6), check_every, between)
    R = _solve(nh, T, max_iters, tol2=tol2, check_every=check_every, trace=False)
    mgd.check_cg_stop(R, seq, tol2, want, label=f"{name}: ")


def test_a_converged_start_runs_no_iteration(nh):
    T = _case(nh, "3d")
    x, r, r32, z32, rr0_ref = rst.store_residual(T.P, T.x0, T.b)
    R = _solve(nh, T, 5, tol2=2.0 * rr0_ref[0])
    done, rr0, rr_last, trace = R.res
    assert (done, R.counts, R.rz0, trace.shape) == (0, (0, 0, 0, 0), 0.0, (0, 3))
    assert rr0 == rr_last and abs(rr0 - rr0_ref[0]) <= rr0_ref[1]
    assert bits_equal(R.x, T.x0) and bits_equal(R.b, T.b)
    # r, r32 and z32 hold what the set-up's step 2 stored
    assert bits_equal(R.r, r) and bits_equal(R.r32, r32) and bits_equal(R.z32, z32)
    # max_iters = 0: rr_0 is still formed
    R = _solve(nh, T, 0, trace=False)
    assert R.res == (0, rr0, rr0) and R.counts == (0, 0, 0, 0) and bits_equal(R.x, T.x0)


def test_misaligned_fields_run_the_scalar_kernel_forms(nh):
    """x, b, r, p, q one f64 element (8 bytes) and r32, z32, minv_0, q_0 one f32 element (4 bytes) into larger allocations: not
    16-byte aligned, so the grid-stride forms of the update and direction kernels run"""
    _check_replay(nh, _case(nh, "3d"), 3, check_every=2, offset=1, want_counts=(1, 2, 0, 2))


@pytest.mark.parametrize("name", ["2d_tail2", "2d_tail3"])
def test_cell_counts_that_are_no_multiple_of_four_take_the_tail(nh, name):
    """aligned fields of 4 k + 2 and 4 k + 3 cells (4 k + 1: the problems "2d" and "3d" above): the 16-byte forms' groups of
    four, then the tail through one lane"""
    T = _case(nh, name)
    assert int(np.prod(T.P.shape)) % 4 == int(name[-1])
    _check_replay(nh, T, 3, want_counts=(1, 2, 0, 3))


def test_more_cells_than_lanes_take_the_grid_stride_loops_round_again(nh):
    """2 129 920 cells in fields one element off 16-byte alignment: the scalar forms' grid is capped at 256 * 32 workgroups
    (2 097 152 lanes), so 32 768 lanes make a second trip; unequal rims on level 0.  Two iterations of V(1, 1) with two coarse
    sweeps: a wrong stride, or a cell summed twice, shows in the fields, in rz' and in rr'."""
    if "big" not in nh.cache:
        t64, t32 = nh.texts["big"]
        T = Case()
        T.P = mx.Problem(rst.Operator(t64), _star_levels(BIG_OMEGA, 2, 6.0 / 7.0, BIG_RIMS, t32))
        T.entry64, T.entries32 = None, [None, None]
        nh.cache["big"] = _finish(nh, T, (t64, t32))
    _check_replay(nh, nh.cache["big"], 2, check_every=2, offset=1, sweeps=1, coarse_sweeps=2, want_counts=(2, 0, 0, 1))


def test_nonzero_dirichlet_rim(nh):
    T = _case(nh, "3d", rim=True)
    R = _check_replay(nh, T, 2)
    outside = np.ones(T.P.shape, bool)
    outside[T.P.where] = False
    assert np.count_nonzero(T.x0[outside]) > 0 and bits_equal(R.x[outside], T.x0[outside])
    zero = _solve(nh, _case(nh, "3d"), 2)
    assert not bits_equal(R.x, zero.x)        # the rim values did enter, through A(x)


def test_two_input_operator_with_a_coefficient_per_level(nh):
    """pcg_cases.pcg_module: an f64 coefficient on the outer level, f32 coefficients per inner level (the f64 one narrowed,
    injected to the coarse grid in numpy): in_rest of the outer level and of every inner level"""
    if "pcg" not in nh.cache:
        t64, t32 = nh.texts["pcg"]
        shapes = mgc.level_shapes(PCG_OMEGA, 2)
        w64 = pc.w_field(shapes[0][0], D, values=(0.0, 1.0, 2.0, 4.0))
        w = [w64.astype(S)]
        wc = np.zeros(shapes[1][0], S)
        wc[shapes[1][1]] = w[0][shapes[0][1]][1::2, 1::2, 1::2]     # the coarse cell j sits on the fine cell 2 j + 1
        w.append(wc)
        levels = []
        for l, (text, (shape, where), wl) in enumerate(zip(t32, shapes, w)):
            minv = np.full(shape, 0.0 if l == 0 else np.nan, S)
            minv[where] = (S(0.8) / (S(12.0) + wl[where])).astype(S)     # pcg_module's diagonal is 4 rank + w
            levels.append(rst.Level(rst.Operator(text, wl), shape, where, minv, S))
        T = Case()
        T.P = mx.Problem(rst.Operator(t64, w64), levels)
        T.entry64, T.entries32 = None, [None, None]
        F = nh.fields.DeviceField
        T.others64, T.others32 = [F.from_numpy(w64)], [[F.from_numpy(wl)] for wl in w]
        nh.cache["pcg"] = _finish(nh, T, (t64, t32))
    R = _check_replay(nh, nh.cache["pcg"], 3, want_counts=(1, 2, 0, 3))
    assert R.res[2] < R.res[1]


def test_builtin_bodies_on_both_level_zeros(nh):
    """the outer operator is the built-in f64 7-point body (fn = NULL: its dot-monitored launch is
    neptune_hip_apply_builtin_dot), the inner level 0 the built-in f32 27-point body, level 1 a lowered module.  The two level-0
    operators differ -- any f32 operator may precondition; the replay holds bit for bit whatever it is worth"""
    shapes = mgc.level_shapes(BUILTIN_OMEGA, 2)
    T = Case()
    levels = [rst.Level(lambda u: helpers.oracle_entry("3d27", u), shapes[0][0], shapes[0][1],
                        mgc.minv_field(shapes[0][0], shapes[0][1], S, 0.125, outside=0.0), S),
              rst.Level(rst.Operator(nh.texts["builtin"][1][1]), shapes[1][0], shapes[1][1], mgc.minv_field(shapes[1][0], shapes[1][1], S, 0.8), S)]
    T.P = mx.Problem(lambda u: helpers.oracle_entry("3d7", u), levels)
    T.entry64 = nh.capi.BODY_LAP3D7_F64
    T.entries32 = [nh.capi.BODY_LAP3D27_F32, mgd.entry(nh, nh.texts["builtin"][1][1], False)]
    T.x0, T.b = mgc.problem_fields(T.P.shape, T.P.where, D)
    _check_replay(nh, T, 3, want_counts=(1, 2, 0, 3))


def test_semi_coarsened_inner_hierarchy(nh):
    """Omega = 15 x 31, dim 0 kept between levels 0 and 1 (15 x 31 -> 15 x 15 -> 7 x 7): the kept-axis transfer kernels in f32"""
    if "semi" not in nh.cache:
        t64, t32 = nh.texts["semi"]
        steps = sc.with_axes(SEMI[0], SEMI[1], SEMI[2])
        levels, _ = sc.build_levels(steps, 0.8, S)
        T = Case()
        T.P = mx.Problem(rst.Operator(t64), levels)
        T.entry64, T.entries32 = None, [None] * len(levels)
        nh.cache["semi"] = _finish(nh, T, (t64, t32))
    T = nh.cache["semi"]
    dev = mx.device_problem(nh, T.P, T.entry64, T.entries32, T.x0, T.b)
    assert dev.h.coarsened == [(1,), (0, 1)]
    _check_replay(nh, T, 3, want_counts=(1, 2, 0, 3))


def test_line_stage_on_level_1(nh):
    """level 1 smooths with one line stage along dim 1 through the unchanged cycle code; level 0 stays point Jacobi"""
    T = _case(nh, "2d", stage_on_level_1=True)
    R = _check_replay(nh, T, 3, want_counts=(1, 2, 0, 3))
    plain = _solve(nh, _case(nh, "2d"), 3)
    assert not bits_equal(R.x, plain.x)       # the stage did run


def test_reaches_a_residual_beyond_f32s_reach(nh):
    """Omega = 31 x 31 to rr <= 1e-24 rr_0 -- a relative residual of 1e-12, which no f32 field can express -- within the
    iteration count the restatement gives"""
    T = _case(nh, "2d")
    seq = rst.numpy_mgcg(T.P, T.x0, T.b, 40, stop_at=0.0)
    want = next(k for k, v in enumerate(seq) if v <= 1e-24 * seq[0])
    R = _solve(nh, T, want, tol2=1e-24 * seq[0], trace=False)
    done, rr0, rr_last = R.res
    print(f"restatement: {want} iterations; device: {done} iterations, rr_last / rr0 = {rr_last / rr0:.3e}")
    assert done <= want and rr_last <= 1e-24 * rr0
    true = mx.true_residual(T.P, R.x, T.b)
    assert rr_last / 4.0 <= true <= rr_last * 4.0


def test_python_wrapper(nh):
    T = _case(nh, "3d")
    ref = _solve(nh, T, 4)
    dev = mx.device_problem(nh, T.P, T.entry64, T.entries32, T.x0, T.b)
    dev.h.x[0] = dev.h.b[0] = None
    # its defaults: V(2, 2), 8 coarse sweeps, no trace, work fields and r32, z32 of its own, the entry's own dot entry
    res = nh.mg.cg_solve_mixed(dev.outer, dev.h, dev.x, dev.b, max_iters=4)
    assert len(res) == 3 and res == ref.res[:3] and bits_equal(dev.x.numpy(), ref.x)
    assert nh.mg.cg_counts() == (1, 3, 0, 4) and nh.mg.cg_rz0() == ref.rz0
    assert bits_equal(dev.h.b[0].numpy(), ref.r32) and bits_equal(dev.h.x[0].numpy(), ref.z32)
    F = nh.fields.DeviceField
    with pytest.raises(ValueError, match="dot is"):
        nh.mg.cg_solve_mixed(dev.outer, dev.h, dev.x, dev.b, dot="never")
    with pytest.raises(ValueError, match="float64"):
        nh.mg.cg_solve_mixed(dev.outer, dev.h, F.from_numpy(T.x0.astype(S)), dev.b)
    with pytest.raises(ValueError, match="float64"):
        nh.mg.cg_solve_mixed(dev.h.levels[0], dev.h, dev.x, dev.b)
    h64 = nh.mg.Hierarchy([nh.mg.Level(T.entry64, F.from_numpy(np.zeros(L.shape)), mx._bounds(L.where), minv=F.from_numpy(L.minv.astype(D)))
                           for L in T.P.levels])
    with pytest.raises(ValueError, match="float32"):
        nh.mg.cg_solve_mixed(dev.outer, h64, dev.x, dev.b)
    with pytest.raises(ValueError, match="two inner levels"):
        nh.mg.cg_solve_mixed(dev.outer, nh.mg.Hierarchy(dev.h.levels[:1]), dev.x, dev.b)
    lb, ub = mx._bounds(T.P.where)
    smaller = nh.mg.Level(T.entry64, F.from_numpy(np.zeros(T.P.shape)), (lb, [ub[0] - 1] + ub[1:]))
    with pytest.raises(ValueError, match="Omega"):
        nh.mg.cg_solve_mixed(smaller, dev.h, dev.x, dev.b)
    staged = _case(nh, "2d", stage_on_level_1=True)
    sdev = mx.device_problem(nh, staged.P, staged.entry64, staged.entries32, staged.x0, staged.b)
    sdev.h.levels[0].lines = sdev.h.levels[1].lines
    with pytest.raises(ValueError, match="level 0"):
        nh.mg.cg_solve_mixed(sdev.outer, sdev.h, sdev.x, sdev.b)


def test_refusals_on_device_pointers(nh):
    """every refusal leaves every field's bits unchanged: nothing was launched"""
    T = _case(nh, "3d")
    dev = mx.device_problem(nh, T.P, T.entry64, T.entries32, T.x0, T.b)
    h, x, b, work = dev.h, dev.x, dev.b, dev.work
    E, U, lib = nh.capi.EINVAL, nh.capi.EUNSUPPORTED, nh.lib
    x.tensor.fill_(-3.0)
    for f in work:
        f.tensor.fill_(-5.0)
    trace = nh.torch.full((3 * 4 + 16,), -7.0, dtype=nh.torch.float64, device="cuda")
    factors = [nh.fields.DeviceField.from_numpy(np.full(T.P.levels[l].shape, 0.25, S)) for l in (0, 1)]

    def call(change=None, outer=None, n_levels=3, pair=(nh.capi.F64, nh.capi.F32), sweeps=2, coarse=8, max_iters=4, check_every=1,
             stream=None, w=None, tr=None, stage_on=None):
        arr, keep = h._structs(h.x[0], h.b[0])
        out = (nh.capi.MgLevel * 1)()
        out[0].fn, out[0].body, out[0].g = C.cast(T.entry64.fn, C.c_void_p), -1, dev.outer.geom
        out[0].x, out[0].b, out[0].q, out[0].rscale = x.ptr, b.ptr, work[2].ptr, 4.0
        if change:
            change(arr)
        if outer:
            outer(out[0])
        lines = None
        if stage_on is not None:
            lines = (nh.capi.MgLines * 3)()
            lines[stage_on].n_stages = 1
            lines[stage_on].axis[0] = 2
            lines[stage_on].lo[0] = lines[stage_on].inv[0] = lines[stage_on].up[0] = factors[stage_on].ptr
        ptrs = [work[0].ptr, work[1].ptr] if w is None else w
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        st = nh.fields.current_stream_ptr() if stream is None else stream
        rc = lib.neptune_hip_mgcg_solve_mixed(out, pair[0], None, arr, lines, n_levels, pair[1], sweeps, coarse, (C.c_void_p * 2)(*ptrs),
                                              max_iters, check_every, 0.0, tr, st, None, C.byref(done), C.byref(rr0), C.byref(last))
        return rc, done.value, rr0.value, last.value

    R = (E, 0, 0.0, 0.0)
    assert call(n_levels=1) == R and call(n_levels=17) == R and call(sweeps=0) == R and call(coarse=-1) == R
    assert call(check_every=0) == R and call(max_iters=-1) == R
    for pair in ((nh.capi.F64, nh.capi.F64), (nh.capi.F32, nh.capi.F32), (nh.capi.F32, nh.capi.F64)):
        assert call(pair=pair) == R, pair
    wp = [work[0].ptr, work[1].ptr]
    wide = int(np.prod(T.P.shape)) * 8
    for i in range(2):
        assert call(w=wp[:i] + [None] + wp[i + 1:]) == R and call(w=wp[:i] + [wp[i] + 4] + wp[i + 1:]) == R
        assert call(w=wp[:i] + [wp[1 - i] + wide - 8] + wp[i + 1:]) == R
        for field in ("x", "b", "q"):
            assert call(outer=lambda o: setattr(o, field, wp[i] + 8)) == R, (i, field)
        for level in (0, 1):
            for field in ("x", "b", "q", "minv"):
                assert call(lambda a: setattr(a[level], field, wp[i] + 8)) == R, (i, level, field)
        assert call(tr=wp[i] + 16) == R
    for field in ("x", "b", "q"):
        assert call(outer=lambda o: setattr(o, field, None)) == R, field
        assert call(tr=getattr(dev, field).ptr + 8 if field != "q" else work[2].ptr + 8) == R, field
        for level in (0, 1):
            for inner in ("x", "b", "q", "minv"):
                assert call(outer=lambda o: setattr(o, field, getattr(h._structs(h.x[0], h.b[0])[0][level], inner))) == R, (field, level, inner)
    for level in (0, 1):
        for field in ("x", "b", "q", "minv"):
            assert call(tr=getattr(h._structs(h.x[0], h.b[0])[0][level], field) + 8) == R, (level, field)
    assert call(w=[wp[0], trace.data_ptr() + 80], tr=trace.data_ptr()) == R
    assert call(tr=trace.data_ptr() + 4) == R

    def smaller_omega(o):
        o.g.ub[2] -= 1
    assert call(outer=smaller_omega) == R

    def smaller_inner_omega(a):
        a[1].g.ub[2] -= 1
    assert call(smaller_inner_omega) == R
    # a line stage on level 0 is unsupported, on level 1 with a factor field inside p refused
    assert call(stage_on=0) == (U, 0, 0.0, 0.0)
    factors[1], kept = work[1], factors[1]
    assert call(stage_on=1) == R
    factors[1] = kept
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
    assert bool((x.tensor == -3.0).all()) and bits_equal(b.numpy(), T.b) and bool((trace == -7.0).all())
    assert all(bool((f.tensor == -5.0).all()) for f in work)
    assert all(bool(nh.torch.isnan(f.tensor).all()) for f in h.q + h.x + h.b)
    assert nh.mg.cg_counts() == (0, 0, 0, 0) and nh.mg.cg_rz0() == 0.0
