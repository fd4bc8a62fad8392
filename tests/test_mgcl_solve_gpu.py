"""neptune_hip_mg_solve_prolong on cell-centred hierarchies with linear prolongation against the NumPy restatement
of tests/mg_restatement.py, through the device harness of tests/mg_device.py.

No reduction enters a field, so after any number of cycles x_0 and every level's x_l, b_l must equal the restatement's bit
for bit, whatever the launch path (plain launches or the replayed graph of one cycle).  rr_0 and every rr read after a block
must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms (monitor_cases.reference_sum's bound).

Operators, one lowered module per level: mgcc_cases.flux_module (face coefficients, and a diagonal field where a face is
Dirichlet), or, where that would take a fifth input -- rank 3 with a Dirichlet face --, mgcl_cases.star_s_module, the same
operator with unit coefficients in two inputs; rscale = 4, minv = 0.8 / diagonal on Omega; the work fields hold NaN before
every call.  Hierarchies: rank 3, 8 x 16 x 264 -> 4 x 8 x 132 -> 2 x 4 x 66, f64 with mixed faces (Dirichlet on the low face of
dimension 0 and the high face of dimension 2, Neumann elsewhere: the two faces of a dimension follow different rules) and f32
with Neumann faces; rank 2, 16 x 264 -> 8 x 132 -> 4 x 66 with Dirichlet faces, also with linear on pair 0 and constant on pair
1; a halved-plus-kept pair with mixed faces, 8 x 264 -> 8 x 132 -> 4 x 66; Omega 14 -> 7 -> 3, the halved pair linear and the
vertex-centred one as it is.  Stop: the plan hierarchy of 32 x 32 x 32 with Dirichlet faces, the threshold at the geometric
mean of two consecutive values of the restatement's sequence (tests/test_mgcl_host.py pins that it falls 7x per cycle at
least)."""
import ctypes as C

import numpy as np
import pytest

import mg_device as mgd
import mg_restatement as rst
import mgcc_cases as cc
import mgcl_cases as cl
import mglines_cases as lc
from helpers import bits_equal, mismatch_report
from mg_restatement import Halved

pytestmark = pytest.mark.gpu

ALL3, ALL2 = Halved((0, 1, 2)), Halved((0, 1))
MIX3 = [("dirichlet", "neumann"), ("neumann", "neumann"), ("neumann", "dirichlet")]
MIX2 = [("dirichlet", "neumann"), ("neumann", "dirichlet")]


def _steps(omega, pairs, faces, only=None):
    return cl.linear_steps(cc.halved_steps(omega, pairs), rst.rim_of(faces, len(omega)), only)


# name: (the steps [(extents, weights, axes)], faces, dtype, the operator's form: mgcl_cases.flux_levels or .star_levels)
PROBLEMS = {
    "3d_f64": (_steps((8, 16, 264), [ALL3, ALL3], MIX3), MIX3, np.float64, cl.star_levels),
    "3d_f32": (_steps((8, 16, 264), [ALL3, ALL3], "neumann"), "neumann", np.float32, cl.flux_levels),
    "2d_f64": (_steps((16, 264), [ALL2, ALL2], "dirichlet"), "dirichlet", np.float64, cl.flux_levels),
    "first_f64": (_steps((16, 264), [ALL2, ALL2], "dirichlet", only={0}), "dirichlet", np.float64, cl.flux_levels),
    "kept_f64": (_steps((8, 264), [Halved((1,)), ALL2], MIX2), MIX2, np.float64, cl.flux_levels),
    "switch_f64": (_steps((14, 14), [ALL2, (0, 1)], "dirichlet"), "dirichlet", np.float64, cl.flux_levels),
    "stop_f64": (cl.linear_steps(cc.plan((32, 32, 32)), rst.rim_of("dirichlet", 3)), "dirichlet", np.float64, cl.star_levels),
}
DAMP = 0.8


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"), check=("halved", "linear"))
    ns.built = {name: form(steps, DAMP, dtype, faces) for name, (steps, faces, dtype, form) in PROBLEMS.items()}
    mgd.prefetch([(t, False) for _, texts, _ in ns.built.values() for t in texts])
    return ns


def _problem(nh, name):
    def build(P):
        _, P.faces, P.dtype, _ = PROBLEMS[name]
        P.ref, P.texts, P.rests = nh.built[name]
        P.x0, P.b = cl.problem(P.ref, P.faces, P.dtype)
    return mgd.problem(nh, name, build)


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(8, 16, 264), (4, 8, 132), (2, 4, 66)] if name.startswith("3d") else
                                    [(16, 264), (8, 132), (4, 66)])
    assert all(L.axes.halved and L.axes.prolong == "linear" for L in P.ref[:-1])
    mgd.check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_linear_on_the_first_pair_and_constant_on_the_second(nh):
    P = _problem(nh, "first_f64")
    assert [(rst.axes_of(L).kind, rst.axes_of(L).prolong, rst.axes_of(L).restrict) for L in P.ref[:-1]] == [("halved", "linear", "average"), ("halved", "constant", "average")]
    mgd.check_against_reference(nh, P, 3)
    # and it is neither all-linear nor all-constant
    x_first = mgd.reference(P, 3)[2][0]
    assert not bits_equal(x_first, mgd.reference(_problem(nh, "2d_f64"), 3)[2][0])


def test_a_halved_plus_kept_pair(nh):
    P = _problem(nh, "kept_f64")
    assert [L.m for L in P.ref] == [(8, 264), (8, 132), (4, 66)] and [tuple(L.axes) for L in P.ref[:-1]] == [(1,), (0, 1)]
    mgd.check_against_reference(nh, P, 3)


def test_linear_on_the_halved_pair_of_a_hierarchy_that_changes_its_grid_kind(nh):
    """Omega 14 -> 7 -> 3: the first pair halved and linear, the second vertex-centred"""
    P = _problem(nh, "switch_f64")
    assert [L.m for L in P.ref] == [(14, 14), (7, 7), (3, 3)] and [(rst.axes_of(L).kind, rst.axes_of(L).prolong, rst.axes_of(L).restrict) for L in P.ref[:-1]] == [("halved", "linear", "average"), ("coarsened", "constant", "average")]
    mgd.check_against_reference(nh, P, 3)


@pytest.mark.parametrize("name", ["3d_f64", "3d_f32"])
def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch, name):
    mgd.graph_vs_plain(nh, _problem(nh, name), monkeypatch, 5)


def test_a_line_stage_on_level_one(nh, monkeypatch):
    """a line stage along the contiguous dimension on level 1 of the rank-2 Dirichlet hierarchy, every pair linear: the
    composed restatement's bits on both launch paths"""
    P = _problem(nh, "2d_f64")

    def lines(l, entry, like, bounds, others):
        return [nh.mg.line_weights(entry, like, bounds, axis=1, others=others, omega=DAMP, reach=1)] if l == 1 else ()
    # the stage's factors from the operator's own coefficient fields (the boundary faces' coefficients are 0)
    R1, (c0, c1, _) = P.ref[1], P.rests[1]
    up_coef = np.zeros_like(c1)
    up_coef[:, :-1] = c1[:, 1:]
    diag = cc.face_fields(R1.m, P.dtype, P.faces, R1.weights)[1]
    R1.stages = [(1,) + lc.factors(-c1, diag, -up_coef, R1.where, 1, DAMP)]
    try:
        ref_rr0, ref_checks = rst.run(P.ref, P.x0, P.b, 4)
        ref = (ref_rr0, ref_checks, [L.x.copy() for L in P.ref], [L.b.copy() for L in P.ref])
    finally:
        del R1.stages
    assert not bits_equal(ref[2][0], mgd.reference(P, 4)[2][0])          # the stage changes the bits
    for graph in ("1", "0"):
        monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", graph)        # read at every call
        h, x, b, _ = mgd.hierarchy(nh, P, lines=lines)
        assert h.has_lines and h.has_linear
        done, rr0, rr_last, rr_checks = nh.mg.solve(h, x, b, max_cycles=4)
        nh.torch.cuda.synchronize()
        assert done == 4 and nh.mg.counts() == ((1, 3, 4) if graph == "1" else (4, 0, 4))
        mgd.compare(ref, rr0, rr_checks, *mgd.fields_of(h, x, b))


def test_no_array_and_constant_everywhere_are_neptune_hip_mg_solve(nh):
    """prolong = NULL, and kind CONSTANT on every pair whatever the rules hold, give neptune_hip_mg_solve's bits, counts and
    scalars on a hierarchy of halved pairs"""
    P = _problem(nh, "3d_f64")
    (res, xs, bs, counts) = mgd.solve(nh, P, 3, constant=True)
    for make in (lambda n: None, lambda n: (nh.capi.MgProlong * n)()):
        h, x, b, _ = mgd.hierarchy(nh, P, constant=True)
        arr, keep = h._structs(x, b)
        prolong = make(len(h) - 1)
        if prolong is not None:
            for p in prolong:
                p.kind = nh.capi.MG_PROLONG_CONSTANT
                for d in range(3):
                    p.rim_lo[d], p.rim_hi[d] = 7, -7
        rr = (C.c_double * 3)()
        done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        rc = nh.lib.neptune_hip_mg_solve_prolong(arr, None, prolong, len(h), h.dtype, 2, 2, 8, 3, 1, 0.0, rr, None, None, C.byref(done),
                                                 C.byref(rr0), C.byref(last))
        nh.torch.cuda.synchronize()
        assert rc == nh.capi.OK and (done.value, rr0.value, last.value, list(rr)) == res and nh.mg.counts() == counts
        for got, want in zip(sum(mgd.fields_of(h, x, b), []), xs + bs):
            assert bits_equal(got, want), mismatch_report(got, want)
    # ... and these are not the linear solve's bits
    assert not bits_equal(xs[0], mgd.reference(P, 3)[2][0])


def test_refusals_on_device_pointers_leave_every_field(nh):
    P = _problem(nh, "2d_f64")
    h, x, b, _ = mgd.hierarchy(nh, P)
    before = mgd.fields_of(h, x, b)
    arr, keep = h._structs(x, b)
    for l, bad in ((0, dict(kind=2)), (1, dict(kind=-1)), (0, dict(lo=(0, 3, 0))), (1, dict(hi=(-1, 0, 0)))):
        prolong = h._prolong_structs()
        if "kind" in bad:
            prolong[l].kind = bad["kind"]
        for d in range(3):
            if "lo" in bad:
                prolong[l].rim_lo[d] = bad["lo"][d]
            if "hi" in bad:
                prolong[l].rim_hi[d] = bad["hi"][d]
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = nh.lib.neptune_hip_mg_solve_prolong(arr, None, prolong, len(h), h.dtype, 2, 2, 8, 3, 1, 0.0, None, None, None, C.byref(done),
                                                 C.byref(rr0), C.byref(last))
        assert rc == nh.capi.EINVAL and (done.value, rr0.value, last.value) == (0, 0.0, 0.0), (l, bad)
    # the rules of dimension 2 of this rank-2 hierarchy are not read
    prolong = h._prolong_structs()
    for p in prolong:
        p.rim_lo[2], p.rim_hi[2] = 5, -5
    nh.torch.cuda.synchronize()
    for got, want in zip(sum(mgd.fields_of(h, x, b), []), sum(before, [])):
        assert bits_equal(got, want), mismatch_report(got, want)
    rc = nh.lib.neptune_hip_mg_solve_prolong(arr, None, prolong, len(h), h.dtype, 2, 2, 8, 2, 1, 0.0, None, None, None, None, None, None)
    nh.torch.cuda.synchronize()
    assert rc == nh.capi.OK
    assert bits_equal(x.numpy(), mgd.reference(P, 2)[2][0])
    # a hierarchy with a linear pair is not for conjugate gradients
    with pytest.raises(ValueError, match="would not be a symmetric preconditioner"):
        nh.mg.cg_solve(h, x, b)


def test_stops_where_the_definition_says_and_before_constant_prolongation(nh):
    """32 x 32 x 32, Dirichlet faces, the threshold between cycles 5 and 6 of the linear sequence: the device stops at the
    restatement's expected_stop; with constant prolongation the same hierarchy has not got there two cycles later"""
    P = _problem(nh, "stop_f64")
    assert [L.m for L in P.ref] == [(32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3, (2,) * 3]
    tol2, done = mgd.check_stop(nh, P, 1, (5, 6), cycles=7)
    assert done == 6
    (done_c, _, last_c, checks_c), _, _, _ = mgd.solve(nh, P, done + 2, tol2=tol2, constant=True)
    print(f"constant: done = {done_c}, checks = {checks_c}")
    assert done_c == done + 2 > done and last_c > tol2
