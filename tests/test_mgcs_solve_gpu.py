"""neptune_hip_mg_solve_transfer, neptune_hip_mgcg_solve_transfer and neptune_hip_mgcg_solve_mixed_transfer on cell-centred
hierarchies whose pairs restrict by the transposed linear prolongation, against the NumPy restatement of
tests/mgcs_cases.py.

No reduction enters a field, so after any number of cycles x_0 and every level's x_l, b_l must equal the restatement's bit
for bit, whatever the launch path (plain launches or the replayed graph); for MGCG the restatement's recurrences are driven
by the device's own scalars (rz_0 and the trace), which then reproduce x, r, p, z and every level's fields bit for bit.  rr_0
and every rr read after a block must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms
(monitor_cases.reference_sum's bound), and so must every traced scalar.

Operators, one lowered module per level, as in test_mgcl_solve_gpu.py: mgcc_cases.flux_module, or, for rank 3 with a Dirichlet
face, mgcl_cases.star_s_module; rscale = 4, minv = 0.8 / diagonal on Omega; the work fields hold NaN before every call.
Hierarchies: rank 3, 8 x 16 x 264 -> 4 x 8 x 132 -> 2 x 4 x 66, f64 and f32 with mixed faces (Dirichlet on the low face of
dimension 0 and the high face of dimension 2, Neumann elsewhere -- a Dirichlet face keeps the operator definite, so r . z stays
positive in f32); rank 2, 16 x 264 -> 8 x 132 -> 4 x 66 with Dirichlet faces, also with the symmetric linear pair on pair 0 and
the constant one on pair 1, and `crossed`: constant prolongation with linear restriction on pair 0, linear prolongation with
averaging restriction on pair 1 (plain cycles only); a halved-plus-kept pair with mixed faces, 8 x 264 -> 8 x 132 -> 4 x 66.
Stop: the plan hierarchy of 32 x 32 x 32 with Dirichlet faces under V(1, 1)."""
import ctypes as C

import numpy as np
import pytest

import mg_restatement as rst
import mgcc_cases as cc
import mgcgmixed_cases as mx
import mgcl_cases as cl
import mgcs_cases as cs
import mglines_cases as lc
from helpers import bits_equal, mismatch_report
from mg_restatement import Halved, Transfers

pytestmark = pytest.mark.gpu

ALL3, ALL2 = Halved((0, 1, 2)), Halved((0, 1))
MIX3 = [("dirichlet", "neumann"), ("neumann", "neumann"), ("neumann", "dirichlet")]
MIX2 = [("dirichlet", "neumann"), ("neumann", "dirichlet")]


def _steps(omega, pairs, faces, only=None):
    return cs.transfer_steps(cc.halved_steps(omega, pairs), rst.rim_of(faces, len(omega)), only=only)


def _crossed():
    rim = rst.rim_of("dirichlet", 2)
    (m0, w0, a0), (m1, w1, a1), last = cc.halved_steps((16, 264), [ALL2, ALL2])
    return [(m0, w0, Transfers(a0, rim, "constant", "linear")), (m1, w1, Transfers(a1, rim, "linear", "average")), last]


# name: (the steps [(extents, weights, axes)], faces, dtype, the operator's form: mgcl_cases.flux_levels or .star_levels)
PROBLEMS = {
    "3d_f64": (_steps((8, 16, 264), [ALL3, ALL3], MIX3), MIX3, np.float64, cl.star_levels),
    "3d_f32": (_steps((8, 16, 264), [ALL3, ALL3], MIX3), MIX3, np.float32, cl.star_levels),
    "2d_f64": (_steps((16, 264), [ALL2, ALL2], "dirichlet"), "dirichlet", np.float64, cl.flux_levels),
    "first_f64": (_steps((16, 264), [ALL2, ALL2], "dirichlet", only={0}), "dirichlet", np.float64, cl.flux_levels),
    "crossed_f64": (_crossed(), "dirichlet", np.float64, cl.flux_levels),
    "kept_f64": (_steps((8, 264), [Halved((1,)), ALL2], MIX2), MIX2, np.float64, cl.flux_levels),
    "const3d_f64": (cc.halved_steps((8, 16, 264), [ALL3, ALL3]), MIX3, np.float64, cl.star_levels),
    "stop_f64": (cs.transfer_steps(cc.plan((32, 32, 32)), rst.rim_of("dirichlet", 3)), "dirichlet", np.float64, cl.star_levels),
    "stop_const_f64": (cc.plan((32, 32, 32)), "dirichlet", np.float64, cl.star_levels),
}
DAMP = 0.8


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    import os
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache"))
    from neptune_hip import _capi, apply, fields, lowering, multigrid

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering, ns.mg = torch, _capi, apply, fields, lowering, multigrid
    ns.lib = _capi.load()
    assert hasattr(ns.lib, "neptune_hip_mgcg_solve_transfer")
    ns.lib.neptune_hip_init(0)
    ns.built = {name: form(steps, DAMP, dtype, faces) for name, (steps, faces, dtype, form) in PROBLEMS.items()}
    _prefetch(lowering, [(t, l == 0) for _, texts, _ in ns.built.values() for l, t in enumerate(texts)])
    ns.entries = {}
    ns.cache = {}
    return ns


def _prefetch(lowering, jobs):
    """every module compiled once, side by side (host threads only, nothing is loaded); level 0's with their dot entries"""
    from concurrent.futures import ThreadPoolExecutor

    def one(job):
        try:
            lowering.compile_module(job[0], load=False, dot_entries=job[1])
        except Exception:       # noqa: BLE001 - the test that needs this module shows the diagnostic
            pass
    with ThreadPoolExecutor(max_workers=12) as pool:
        list(pool.map(one, dict.fromkeys(jobs)))


def _entry(nh, text, dot):
    key = (text, dot)
    if key not in nh.entries:
        nh.entries[key] = (nh.lowering.compile_module(text, dot_entries=True).dot_entry("entry") if dot else
                           nh.lowering.compile_module(text).geom_entry("entry"))
    return nh.entries[key]


class Problem:
    pass


def _problem(nh, name):
    """the compiled operators, the restatement's levels, x0 and b: built once per problem, x0 and b left unchanged"""
    if name not in nh.cache:
        P = Problem()
        _, P.faces, P.dtype, _ = PROBLEMS[name]
        P.ref, P.texts, P.rests = nh.built[name]
        P.entries = [_entry(nh, t, l == 0) for l, t in enumerate(P.texts)]
        P.x0, P.b = cl.problem(P.ref, P.faces, P.dtype)
        for a in (P.x0, P.b):
            a.setflags(write=False)
        P.runs = {}
        nh.cache[name] = P
    return nh.cache[name]


def _reference(P, cycles, check_every=1):
    """the restatement's run, computed once per schedule and left unchanged: -> (rr0, checks, [x_l], [b_l])"""
    key = (cycles, check_every)
    if key not in P.runs:
        rr0, checks = rst.run(P.ref, P.x0, P.b, cycles, check_every=check_every)
        P.runs[key] = (rr0, checks, [L.x.copy() for L in P.ref], [L.b.copy() for L in P.ref])
    return P.runs[key]


def _setting(axes):
    if getattr(axes, "rim", None) is not None:           # a pair with its transfers chosen
        out = dict(prolong=axes.prolong, restrict=axes.restrict)
        if axes.prolong == "linear" or axes.restrict == "linear":
            out["faces"] = rst.faces_of(axes.rim)
        return out
    return {}


def _levels(nh, P, lines=None):
    F = nh.fields.DeviceField
    levels = []
    for l, R in enumerate(P.ref):
        like = F.from_numpy(np.zeros(R.shape, P.dtype))
        bounds = ([s.start for s in R.where], [s.stop for s in R.where])
        others = [F.from_numpy(a) for a in P.rests[l]]
        stages = lines(l, P.entries[l], like, bounds, others) if lines else ()
        levels.append(nh.mg.Level(P.entries[l], like, bounds, others=others, minv=F.from_numpy(R.minv), rscale=R.rscale, lines=stages,
                                  **_setting(R.axes)))
    return levels


def _hierarchy(nh, P, lines=None):
    """a device hierarchy whose work fields hold NaN, every pair of the restatement with its two transfers; -> (h, x, b, [r, p, z])"""
    F = nh.fields.DeviceField
    h = nh.mg.Hierarchy(_levels(nh, P, lines))
    assert h.halved == [tuple(R.axes) if rst.axes_of(R).halved else () for R in P.ref[:-1]]
    assert [(L.linear, L.restrict_linear) for L in h.levels[:-1]] == [
        (getattr(R.axes, "prolong", "") == "linear", getattr(R.axes, "restrict", "") == "linear") for R in P.ref[:-1]]
    nan = lambda f: F.from_numpy(np.full(f.shape, np.nan, P.dtype))
    h.q = [nan(f) for f in h.q]
    h.x = [None] + [nan(f) for f in h.x[1:]]
    h.b = [None] + [nan(f) for f in h.b[1:]]
    return h, F.from_numpy(P.x0), F.from_numpy(P.b), [nan(h.q[0]) for _ in range(3)]


def _fields(h, x, b):
    return [x.numpy()] + [f.numpy() for f in h.x[1:]], [b.numpy()] + [f.numpy() for f in h.b[1:]]


def _solve(nh, P, max_cycles, tol2=0.0, check_every=1):
    h, x, b, _ = _hierarchy(nh, P)
    res = nh.mg.solve(h, x, b, max_cycles=max_cycles, tol2=tol2, check_every=check_every)
    nh.torch.cuda.synchronize()
    return (res,) + _fields(h, x, b) + (nh.mg.counts(),)


def _compare(ref, got_rr0, got_checks, xs, bs):
    ref_rr0, ref_checks, ref_x, ref_b = ref
    print(f"rr0 = {got_rr0!r} (terms' sum {ref_rr0[0]!r}, bound {ref_rr0[1]:.3e})")
    assert abs(got_rr0 - ref_rr0[0]) <= ref_rr0[1]
    assert len(got_checks) == len(ref_checks)
    for k, (got, (want, bound)) in enumerate(zip(got_checks, ref_checks)):
        print(f"  check {k}: rr = {got!r} (terms' sum {want!r}, bound {bound:.3e})")
        assert abs(got - want) <= bound
    for l, (got, want) in enumerate(zip(xs, ref_x)):
        assert bits_equal(got, want), f"x_{l}: " + mismatch_report(got, want)
    for l, (got, want) in enumerate(zip(bs, ref_b)):
        assert bits_equal(got, want), f"b_{l}: " + mismatch_report(got, want)


def _check_against_reference(nh, P, cycles, want_counts=None):
    (done, rr0, rr_last, rr_checks), xs, bs, counts = _solve(nh, P, cycles)
    assert done == cycles and rr_last == rr_checks[-1]
    if want_counts is not None:
        assert counts == want_counts, counts
    _compare(_reference(P, cycles), rr0, rr_checks, xs, bs)


# ---------------------------------------------------------------- plain cycles
@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(8, 16, 264), (4, 8, 132), (2, 4, 66)] if name.startswith("3d") else
                                    [(16, 264), (8, 132), (4, 66)])
    assert all(L.axes.halved and L.axes.symmetric and L.axes.restrict == "linear" for L in P.ref[:-1])
    _check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_the_symmetric_pair_first_and_the_constant_pair_second(nh):
    P = _problem(nh, "first_f64")
    assert [(rst.axes_of(L).kind, rst.axes_of(L).prolong, rst.axes_of(L).restrict) for L in P.ref[:-1]] == [("halved", "linear", "linear"), ("halved", "constant", "average")]
    _check_against_reference(nh, P, 3)
    assert not bits_equal(_reference(P, 3)[2][0], _reference(_problem(nh, "2d_f64"), 3)[2][0])


def test_any_combination_per_pair_in_plain_cycles(nh):
    """constant prolongation with linear restriction on pair 0, linear prolongation with averaging restriction on pair 1"""
    P = _problem(nh, "crossed_f64")
    assert [(L.axes.prolong, L.axes.restrict) for L in P.ref[:-1]] == [("constant", "linear"), ("linear", "average")]
    _check_against_reference(nh, P, 3)
    h, x, b, work = _hierarchy(nh, P)
    assert not h.symmetric
    with pytest.raises(ValueError, match="would not be a symmetric preconditioner"):
        nh.mg.cg_solve(h, x, b, work=work)


def test_a_halved_plus_kept_pair(nh):
    P = _problem(nh, "kept_f64")
    assert [L.m for L in P.ref] == [(8, 264), (8, 132), (4, 66)] and [tuple(L.axes) for L in P.ref[:-1]] == [(1,), (0, 1)]
    _check_against_reference(nh, P, 3)


# ---------------------------------------------------------------- MGCG
def _cg(nh, P, iters, stages=None, **kw):
    h, x, b, work = _hierarchy(nh, P, stages)
    assert h.symmetric and h.has_linear_restrict
    res = nh.mg.cg_solve(h, x, b, max_iters=iters, trace=True, work=work, **kw)
    nh.torch.cuda.synchronize()
    return res, h, x, work, nh.mg.cg_counts(), nh.mg.cg_rz0()


def _check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks):
    print(f"rr0 = {rr0!r} (terms' sum {rr0_ref[0]!r}, bound {rr0_ref[1]:.3e})  rz0 = {rz0!r} (sum {rz0_ref[0]!r}, bound {rz0_ref[1]:.3e})")
    assert abs(rr0 - rr0_ref[0]) <= rr0_ref[1] and abs(rz0 - rz0_ref[0]) <= rz0_ref[1]
    for k, sums in enumerate(checks):
        print(f"  k={k}: " + "  ".join(f"{nm} = {trace[k][c]!r} (sum {s!r}, bound {bd:.3e})"
                                        for c, (nm, (s, bd)) in enumerate(zip(("pq", "rz'", "rr'"), sums))))
        for c, (s, bd) in enumerate(sums):
            assert abs(float(trace[k][c]) - s) <= bd


def _check_levels(h, ref):
    for l in range(1, len(ref)):
        for nm, got, want in ((f"x_{l}", h.x[l].numpy(), ref[l].x), (f"b_{l}", h.b[l].numpy(), ref[l].b)):
            assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)


def _check_replay(nh, P, iters):
    (done, rr0, rr_last, trace), h, x, work, counts, rz0 = _cg(nh, P, iters)
    assert done == iters and trace.shape == (iters, 3)
    print(f"counts = {counts}")
    assert (counts[0], counts[1], counts[3]) == ((iters, 0, iters) if iters <= 2 else (1, iters - 1, iters)), counts
    st, checks, rr0_ref, rz0_ref, _ = rst.replay(P.ref, P.x0, P.b, rz0, trace)
    rx, rr, rp, rz = st.x, st.r, st.p, st.z
    _check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks)
    assert rr_last == float(trace[-1][2])
    assert all(float(row[1]) > 0 for row in trace) and rz0 > 0                         # the preconditioner is positive
    for nm, got, want in (("x", x.numpy(), rx), ("r", work[0].numpy(), rr), ("p", work[1].numpy(), rp), ("z", work[2].numpy(), rz)):
        assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)
    _check_levels(h, P.ref)


@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", ["3d_f32", "3d_f64", "2d_f64"])
def test_mgcg_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    _check_replay(nh, _problem(nh, name), iters)


def test_mgcg_with_the_symmetric_pair_first_and_the_constant_pair_second(nh):
    _check_replay(nh, _problem(nh, "first_f64"), 3)


def test_mgcg_on_a_halved_plus_kept_pair(nh):
    _check_replay(nh, _problem(nh, "kept_f64"), 3)


def test_mgcg_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    P = _problem(nh, "3d_f64")
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", graph)        # read at every call
        (done, rr0, rr_last, trace), h, x, work, counts, rz0 = _cg(nh, P, 5)
        assert (counts[0], counts[1], counts[3]) == ((1, 4, 5) if graph == "1" else (5, 0, 5)), counts
        out.append(((done, rr0, rr_last, rz0), [trace, x.numpy()] + [f.numpy() for f in work] + [f.numpy() for f in h.x[1:] + h.b[1:]]))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1], out[1][1]):
        assert bits_equal(a, b), mismatch_report(a, b)


def _cg_sequence(P, sweeps):
    """r . r of the restatement's recurrences (numpy's own sums) down to 1e-16 rr_0, computed once: -> (seq, tol2)"""
    key = ("cg_seq", sweeps)
    if key not in P.runs:
        rr0 = rst.numpy_mgcg(P.ref, P.x0, P.b, 0, sweeps)[0]
        P.runs[key] = (rst.numpy_mgcg(P.ref, P.x0, P.b, 40, sweeps, stop_at=1e-16 * rr0), 1e-16 * rr0)
    return P.runs[key]


@pytest.mark.parametrize("name", ["2d_f64", "kept_f64"])
def test_mgcg_iteration_count(nh, name):
    """to 1e-16 rr_0: the count of the restatement's recurrences, whose r . r at the stop and one iteration before must be a
    factor of 2 either side of the threshold, so that the count cannot hinge on a summation order"""
    P = _problem(nh, name)
    seq, tol2 = _cg_sequence(P, 2)
    n = len(seq) - 1
    print(f"seq = {seq}, tol2 = {tol2!r}")
    assert 1 <= n < 40 and seq[n] <= 0.5 * tol2 and seq[n - 1] >= 2.0 * tol2, "precondition on the restatement"
    h, x, b, work = _hierarchy(nh, P)
    done, rr0, rr_last = nh.mg.cg_solve(h, x, b, max_iters=40, tol2=tol2, work=work)
    nh.torch.cuda.synchronize()
    print(f"done = {done}, rr0 = {rr0!r}, rr_last = {rr_last!r}")
    assert done == n and rr_last <= tol2 < rr0
    assert np.isfinite(x.numpy()).all()


def test_mgcg_with_a_line_stage_on_level_one(nh):
    """cg_solve(lines=True) with a line stage along the contiguous dimension on level 1 of the rank-2 Dirichlet hierarchy, every
    pair symmetric linear: the composed restatement, driven by the device's scalars, reproduces every field"""
    P = _problem(nh, "2d_f64")

    def lines(l, entry, like, bounds, others):
        return [nh.mg.line_weights(entry, like, bounds, axis=1, others=others, omega=DAMP, reach=1)] if l == 1 else ()
    R1, (c0, c1, _) = P.ref[1], P.rests[1]
    up_coef = np.zeros_like(c1)
    up_coef[:, :-1] = c1[:, 1:]
    diag = cc.face_fields(R1.m, P.dtype, P.faces, R1.weights)[1]
    R1.stages = [(1,) + lc.factors(-c1, diag, -up_coef, R1.where, 1, DAMP)]
    try:
        (done, rr0, rr_last, trace), h, x, work, counts, rz0 = _cg(nh, P, 4, lines, lines=True)
        assert h.has_lines and done == 4 and (counts[0], counts[1], counts[3]) == (1, 3, 4)
        st, checks, rr0_ref, rz0_ref, _ = rst.replay(P.ref, P.x0, P.b, rz0, trace)
        _check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks)
        for nm, got, want in (("x", x.numpy(), st.x), ("r", work[0].numpy(), st.r), ("p", work[1].numpy(), st.p), ("z", work[2].numpy(), st.z)):
            assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)
        _check_levels(h, P.ref)
    finally:
        del R1.stages
    # the stage changes the bits
    assert not bits_equal(st.x, rst.replay(P.ref, P.x0, P.b, rz0, trace)[0].x)


def test_mixed_precision_against_the_composed_restatement(nh):
    """f64 conjugate gradients on the f64 operator around the f32 cycle of the symmetric linear hierarchy"""
    P64, P32 = _problem(nh, "3d_f64"), _problem(nh, "3d_f32")
    F = nh.fields.DeviceField
    outer = _levels(nh, P64)[0]
    inner = nh.mg.Hierarchy(_levels(nh, P32))
    assert inner.symmetric and inner.has_linear_restrict
    x, b = F.from_numpy(P64.x0), F.from_numpy(P64.b)
    work = [F.from_numpy(np.full(P64.x0.shape, np.nan)) for _ in range(3)]
    nan32 = lambda f: F.from_numpy(np.full(f.shape, np.nan, np.float32))
    inner.q = [nan32(f) for f in inner.q]
    inner.x = [nan32(inner.q[0])] + [nan32(f) for f in inner.x[1:]]
    inner.b = [nan32(inner.q[0])] + [nan32(f) for f in inner.b[1:]]
    done, rr0, rr_last, trace = nh.mg.cg_solve_mixed(outer, inner, x, b, max_iters=4, trace=True, work=work)
    nh.torch.cuda.synchronize()
    rz0 = nh.mg.cg_rz0()
    assert done == 4 and trace.shape == (4, 3) and rr_last < rr0
    R = mx.Problem(P64.ref[0].A, P32.ref)
    st, checks, rr0_ref, rz0_ref, _ = rst.replay(R, P64.x0, P64.b, rz0, trace)
    _check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks)
    for nm, got, want in (("x", x.numpy(), st.x), ("r", work[0].numpy(), st.r), ("p", work[1].numpy(), st.p),
                          ("r32", inner.b[0].numpy(), st.r32), ("z32", inner.x[0].numpy(), st.z32)):
        assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)
    _check_levels(inner, P32.ref)


# ---------------------------------------------------------------- the default array is the existing entry
def _default_array(nh, n):
    arr = (nh.capi.MgTransfer * n)()
    for t in arr:
        t.prolong, t.restrict_kind = nh.capi.MG_PROLONG_CONSTANT, nh.capi.MG_RESTRICT_AVERAGE
        for d in range(3):
            t.rim_lo[d], t.rim_hi[d] = 7, -7           # not read
    return arr


def test_no_array_and_the_default_everywhere_are_the_existing_entries(nh):
    """transfer = NULL, and CONSTANT / AVERAGE on every pair whatever the rules hold, give the bits, counts and scalars of
    neptune_hip_mg_solve and neptune_hip_mgcg_solve on a hierarchy of halved pairs"""
    P = _problem(nh, "const3d_f64")
    (res, xs, bs, counts) = _solve(nh, P, 3)
    for make in (lambda n: None, lambda n: _default_array(nh, n)):
        h, x, b, _ = _hierarchy(nh, P)
        arr, keep = h._structs(x, b)
        rr = (C.c_double * 3)()
        done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        rc = nh.lib.neptune_hip_mg_solve_transfer(arr, None, make(len(h) - 1), len(h), h.dtype, 2, 2, 8, 3, 1, 0.0, rr, None, None,
                                                  C.byref(done), C.byref(rr0), C.byref(last))
        nh.torch.cuda.synchronize()
        assert rc == nh.capi.OK and (done.value, rr0.value, last.value, list(rr)) == res and nh.mg.counts() == counts
        for got, want in zip(sum(_fields(h, x, b), []), xs + bs):
            assert bits_equal(got, want), mismatch_report(got, want)
    h, x, b, work = _hierarchy(nh, P)
    want = nh.mg.cg_solve(h, x, b, max_iters=3, trace=True, work=work)
    nh.torch.cuda.synchronize()
    want_fields = [x.numpy()] + [f.numpy() for f in work] + sum(_fields(h, x, b), [])[1:]
    want_counts, want_rz0 = nh.mg.cg_counts(), nh.mg.cg_rz0()
    for make in (lambda n: None, lambda n: _default_array(nh, n)):
        h, x, b, work = _hierarchy(nh, P)
        arr, keep = h._structs(x, b)
        tr = nh.torch.zeros(9, dtype=nh.torch.float64, device="cuda")
        warr = (C.c_void_p * 3)(*[f.ptr for f in work])
        entry = h.levels[0].entry
        done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        rc = nh.lib.neptune_hip_mgcg_solve_transfer(arr, None, make(len(h) - 1), len(h), h.dtype, C.cast(entry.fn_dot, C.c_void_p), 2, 8, warr,
                                                    3, 1, 0.0, tr.data_ptr(), None, None, C.byref(done), C.byref(rr0), C.byref(last))
        nh.torch.cuda.synchronize()
        assert rc == nh.capi.OK and (done.value, rr0.value, last.value) == want[:3]
        assert nh.mg.cg_counts() == want_counts and nh.mg.cg_rz0() == want_rz0
        assert bits_equal(tr.cpu().numpy().reshape(-1, 3), want[3])
        for got, ref in zip([x.numpy()] + [f.numpy() for f in work] + sum(_fields(h, x, b), [])[1:], want_fields):
            assert bits_equal(got, ref), mismatch_report(got, ref)
    # ... and these are not the symmetric pair's bits
    assert not bits_equal(xs[0], _reference(_problem(nh, "3d_f64"), 3)[2][0])


# ---------------------------------------------------------------- refusals
def test_refusals_on_device_pointers_leave_every_field(nh):
    P = _problem(nh, "2d_f64")
    h, x, b, work = _hierarchy(nh, P)
    before = sum(_fields(h, x, b), []) + [f.numpy() for f in work]
    arr, keep = h._structs(x, b)
    warr = (C.c_void_p * 3)(*[f.ptr for f in work])
    lin, avg, const = nh.capi.MG_RESTRICT_LINEAR, nh.capi.MG_RESTRICT_AVERAGE, nh.capi.MG_PROLONG_CONSTANT

    def plain(transfer):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = nh.lib.neptune_hip_mg_solve_transfer(arr, None, transfer, len(h), h.dtype, 2, 2, 8, 3, 1, 0.0, None, None, None, C.byref(done),
                                                  C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc

    def cg(transfer):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = nh.lib.neptune_hip_mgcg_solve_transfer(arr, None, transfer, len(h), h.dtype, None, 2, 8, warr, 3, 1, 0.0, None, None, None,
                                                    C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc
    E = nh.capi.EINVAL
    for l, bad in ((0, dict(restrict_kind=2)), (1, dict(restrict_kind=-1)), (0, dict(prolong=2)), (0, dict(lo=(0, 3, 0))),
                   (1, dict(hi=(-1, 0, 0)))):
        transfer = h._transfer_structs()
        for key in ("restrict_kind", "prolong"):
            if key in bad:
                setattr(transfer[l], key, bad[key])
        for d in range(3):
            if "lo" in bad:
                transfer[l].rim_lo[d] = bad["lo"][d]
            if "hi" in bad:
                transfer[l].rim_hi[d] = bad["hi"][d]
        assert plain(transfer) == E and cg(transfer) == E, (l, bad)
    # an asymmetric pair: refused by the CG entry only (the plain one runs it: test_any_combination_per_pair_in_plain_cycles)
    for l, (prolong, restrict) in ((0, (const, lin)), (1, (1, avg))):
        transfer = h._transfer_structs()
        transfer[l].prolong, transfer[l].restrict_kind = prolong, restrict
        assert cg(transfer) == E, (l, prolong, restrict)
    nh.torch.cuda.synchronize()
    for got, want in zip(sum(_fields(h, x, b), []) + [f.numpy() for f in work], before):
        assert bits_equal(got, want), mismatch_report(got, want)
    # the rules of dimension 2 of this rank-2 hierarchy are not read
    transfer = h._transfer_structs()
    for t in transfer:
        t.rim_lo[2], t.rim_hi[2] = 5, -5
    rc = nh.lib.neptune_hip_mg_solve_transfer(arr, None, transfer, len(h), h.dtype, 2, 2, 8, 2, 1, 0.0, None, None, None, None, None, None)
    nh.torch.cuda.synchronize()
    assert rc == nh.capi.OK
    assert bits_equal(x.numpy(), _reference(P, 2)[2][0])


# ---------------------------------------------------------------- the stop
def test_v11_stops_at_the_restatements_iteration_and_before_the_constant_pair(nh):
    """32 x 32 x 32, Dirichlet faces, V(1, 1), to 1e-16 rr_0: with the symmetric linear pair the device stops at the iteration
    of the restatement's recurrences (whose r . r at the stop and one iteration before are a factor of 2 either side of the
    threshold); with the constant pair the same solve has not stopped by then"""
    P, Pc = _problem(nh, "stop_f64"), _problem(nh, "stop_const_f64")
    assert [L.m for L in P.ref] == [(32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3, (2,) * 3]
    seq, tol2 = _cg_sequence(P, 1)
    n = len(seq) - 1
    print(f"seq = {seq}, tol2 = {tol2!r}")
    assert 1 <= n < 40 and seq[n] <= 0.5 * tol2 and seq[n - 1] >= 2.0 * tol2, "precondition on the restatement"
    h, x, b, work = _hierarchy(nh, P)
    done, rr0, rr_last = nh.mg.cg_solve(h, x, b, sweeps=1, max_iters=40, tol2=tol2, work=work)
    nh.torch.cuda.synchronize()
    print(f"symmetric linear: done = {done}, rr0 = {rr0!r}, rr_last = {rr_last!r}")
    assert done == n and rr_last <= tol2 < rr0
    assert bits_equal(P.b, Pc.b)
    h, x, b, work = _hierarchy(nh, Pc)
    done_c, rr0_c, last_c = nh.mg.cg_solve(h, x, b, sweeps=1, max_iters=n, tol2=tol2, work=work)
    nh.torch.cuda.synchronize()
    print(f"constant: done = {done_c}, rr_last = {last_c!r}")
    assert done_c == n and last_c > tol2 and rr0_c == rr0
