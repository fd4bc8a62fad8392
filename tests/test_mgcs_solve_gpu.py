"""neptune_hip_mg_solve_transfer, neptune_hip_mgcg_solve_transfer and neptune_hip_mgcg_solve_mixed_transfer on cell-centred
hierarchies whose pairs restrict by the transposed linear prolongation, against the NumPy restatement of
tests/mg_restatement.py, through the device harness of tests/mg_device.py.

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

import mg_device as mgd
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
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"), check=("halved", "transfers"))
    assert hasattr(ns.lib, "neptune_hip_mgcg_solve_transfer")
    ns.built = {name: form(steps, DAMP, dtype, faces) for name, (steps, faces, dtype, form) in PROBLEMS.items()}
    mgd.prefetch([(t, l == 0) for _, texts, _ in ns.built.values() for l, t in enumerate(texts)])
    return ns


def _problem(nh, name):
    def build(P):
        _, P.faces, P.dtype, _ = PROBLEMS[name]
        P.ref, P.texts, P.rests = nh.built[name]
        P.x0, P.b = cl.problem(P.ref, P.faces, P.dtype)
    return mgd.problem(nh, name, build, dots=(0,))


# ---------------------------------------------------------------- plain cycles
@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(8, 16, 264), (4, 8, 132), (2, 4, 66)] if name.startswith("3d") else
                                    [(16, 264), (8, 132), (4, 66)])
    assert all(L.axes.halved and L.axes.symmetric and L.axes.restrict == "linear" for L in P.ref[:-1])
    mgd.check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_the_symmetric_pair_first_and_the_constant_pair_second(nh):
    P = _problem(nh, "first_f64")
    assert [(rst.axes_of(L).kind, rst.axes_of(L).prolong, rst.axes_of(L).restrict) for L in P.ref[:-1]] == [("halved", "linear", "linear"), ("halved", "constant", "average")]
    mgd.check_against_reference(nh, P, 3)
    assert not bits_equal(mgd.reference(P, 3)[2][0], mgd.reference(_problem(nh, "2d_f64"), 3)[2][0])


def test_any_combination_per_pair_in_plain_cycles(nh):
    """constant prolongation with linear restriction on pair 0, linear prolongation with averaging restriction on pair 1"""
    P = _problem(nh, "crossed_f64")
    assert [(L.axes.prolong, L.axes.restrict) for L in P.ref[:-1]] == [("constant", "linear"), ("linear", "average")]
    mgd.check_against_reference(nh, P, 3)
    h, x, b, work = mgd.hierarchy(nh, P)
    assert not h.symmetric
    with pytest.raises(ValueError, match="would not be a symmetric preconditioner"):
        nh.mg.cg_solve(h, x, b, work=work)


def test_a_halved_plus_kept_pair(nh):
    P = _problem(nh, "kept_f64")
    assert [L.m for L in P.ref] == [(8, 264), (8, 132), (4, 66)] and [tuple(L.axes) for L in P.ref[:-1]] == [(1,), (0, 1)]
    mgd.check_against_reference(nh, P, 3)


# ---------------------------------------------------------------- MGCG
def _symmetric(h):
    return h.symmetric and h.has_linear_restrict


def _counts(iters):
    """(plain, graph, checks) of `iters` iterations checked every time"""
    return (iters, 0, iters) if iters <= 2 else (1, iters - 1, iters)


def _check_replay(nh, P, iters):
    R = mgd.check_replay(nh, P, iters, want_counts=_counts(iters), any_fallback=True, require=_symmetric)
    assert all(float(row[1]) > 0 for row in R.res[3]) and R.rz0 > 0                    # the preconditioner is positive


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
        R = mgd.cg(nh, P, 5, require=_symmetric)
        assert (R.counts[0], R.counts[1], R.counts[3]) == ((1, 4, 5) if graph == "1" else (5, 0, 5)), R.counts
        out.append(R)
    mgd.same_runs(*out)


@pytest.mark.parametrize("name", ["2d_f64", "kept_f64"])
def test_mgcg_iteration_count(nh, name):
    """to 1e-16 rr_0: the count of the restatement's recurrences (mg_device.check_iteration_count)"""
    _, _, _, x = mgd.check_iteration_count(nh, _problem(nh, name), 40)
    assert np.isfinite(x).all()


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
        R = mgd.cg(nh, P, 4, stages=lines, require=_symmetric, lines=True)
        (done, rr0, rr_last, trace), rz0 = R.res, R.rz0
        assert R.h.has_lines and done == 4 and (R.counts[0], R.counts[1], R.counts[3]) == (1, 3, 4)
        st, checks, rr0_ref, rz0_ref, _ = rst.replay(P.ref, P.x0, P.b, rz0, trace)
        mgd.check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks)
        for nm, got, want in (("x", R.x, st.x), ("r", R.r, st.r), ("p", R.p, st.p), ("z", R.z, st.z)):
            mgd.same(nm, got, want)
        mgd.check_levels(R.xs, R.bs, P.ref)
    finally:
        del R1.stages
    # the stage changes the bits
    assert not bits_equal(st.x, rst.replay(P.ref, P.x0, P.b, rz0, trace)[0].x)


def test_mixed_precision_against_the_composed_restatement(nh):
    """f64 conjugate gradients on the f64 operator around the f32 cycle of the symmetric linear hierarchy"""
    P64, P32 = _problem(nh, "3d_f64"), _problem(nh, "3d_f32")
    outer, inner, x, b, work = mgd.mixed(nh, P64, P32)
    assert _symmetric(inner)
    done, rr0, rr_last, trace = nh.mg.cg_solve_mixed(outer, inner, x, b, max_iters=4, trace=True, work=work)
    nh.torch.cuda.synchronize()
    rz0 = nh.mg.cg_rz0()
    assert done == 4 and trace.shape == (4, 3) and rr_last < rr0
    R = mx.Problem(P64.ref[0].A, P32.ref)
    st, checks, rr0_ref, rz0_ref, _ = rst.replay(R, P64.x0, P64.b, rz0, trace)
    mgd.check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks)
    for nm, got, want in (("x", x.numpy(), st.x), ("r", work[0].numpy(), st.r), ("p", work[1].numpy(), st.p),
                          ("r32", inner.b[0].numpy(), st.r32), ("z32", inner.x[0].numpy(), st.z32)):
        mgd.same(nm, got, want)
    mgd.check_levels(*[[f.numpy() for f in fs[1:]] for fs in (inner.x, inner.b)], P32.ref)


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
    (res, xs, bs, counts) = mgd.solve(nh, P, 3)
    for make in (lambda n: None, lambda n: _default_array(nh, n)):
        h, x, b, _ = mgd.hierarchy(nh, P)
        arr, keep = h._structs(x, b)
        rr = (C.c_double * 3)()
        done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        rc = nh.lib.neptune_hip_mg_solve_transfer(arr, None, make(len(h) - 1), len(h), h.dtype, 2, 2, 8, 3, 1, 0.0, rr, None, None,
                                                  C.byref(done), C.byref(rr0), C.byref(last))
        nh.torch.cuda.synchronize()
        assert rc == nh.capi.OK and (done.value, rr0.value, last.value, list(rr)) == res and nh.mg.counts() == counts
        for got, want in zip(sum(mgd.fields_of(h, x, b), []), xs + bs):
            assert bits_equal(got, want), mismatch_report(got, want)
    h, x, b, work = mgd.hierarchy(nh, P)
    want = nh.mg.cg_solve(h, x, b, max_iters=3, trace=True, work=work)
    nh.torch.cuda.synchronize()
    want_fields = [x.numpy()] + [f.numpy() for f in work] + sum(mgd.fields_of(h, x, b), [])[1:]
    want_counts, want_rz0 = nh.mg.cg_counts(), nh.mg.cg_rz0()
    for make in (lambda n: None, lambda n: _default_array(nh, n)):
        h, x, b, work = mgd.hierarchy(nh, P)
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
        for got, ref in zip([x.numpy()] + [f.numpy() for f in work] + sum(mgd.fields_of(h, x, b), [])[1:], want_fields):
            assert bits_equal(got, ref), mismatch_report(got, ref)
    # ... and these are not the symmetric pair's bits
    assert not bits_equal(xs[0], mgd.reference(_problem(nh, "3d_f64"), 3)[2][0])


# ---------------------------------------------------------------- refusals
def test_refusals_on_device_pointers_leave_every_field(nh):
    P = _problem(nh, "2d_f64")
    h, x, b, work = mgd.hierarchy(nh, P)
    before = sum(mgd.fields_of(h, x, b), []) + [f.numpy() for f in work]
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
    for got, want in zip(sum(mgd.fields_of(h, x, b), []) + [f.numpy() for f in work], before):
        assert bits_equal(got, want), mismatch_report(got, want)
    # the rules of dimension 2 of this rank-2 hierarchy are not read
    transfer = h._transfer_structs()
    for t in transfer:
        t.rim_lo[2], t.rim_hi[2] = 5, -5
    rc = nh.lib.neptune_hip_mg_solve_transfer(arr, None, transfer, len(h), h.dtype, 2, 2, 8, 2, 1, 0.0, None, None, None, None, None, None)
    nh.torch.cuda.synchronize()
    assert rc == nh.capi.OK
    assert bits_equal(x.numpy(), mgd.reference(P, 2)[2][0])


# ---------------------------------------------------------------- the stop
def test_v11_stops_at_the_restatements_iteration_and_before_the_constant_pair(nh):
    """32 x 32 x 32, Dirichlet faces, V(1, 1), to 1e-16 rr_0: with the symmetric linear pair the device stops at the iteration
    of the restatement's recurrences (whose r . r at the stop and one iteration before are a factor of 2 either side of the
    threshold); with the constant pair the same solve has not stopped by then"""
    P, Pc = _problem(nh, "stop_f64"), _problem(nh, "stop_const_f64")
    assert [L.m for L in P.ref] == [(32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3, (2,) * 3]
    n, tol2, rr0, _ = mgd.check_iteration_count(nh, P, 40, sweeps=1, label="symmetric linear: ")
    assert bits_equal(P.b, Pc.b)
    h, x, b, work = mgd.hierarchy(nh, Pc)
    done_c, rr0_c, last_c = nh.mg.cg_solve(h, x, b, sweeps=1, max_iters=n, tol2=tol2, work=work)
    nh.torch.cuda.synchronize()
    print(f"constant: done = {done_c}, rr_last = {last_c!r}")
    assert done_c == n and last_c > tol2 and rr0_c == rr0
