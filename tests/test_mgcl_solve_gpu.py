"""neptune_hip_mg_solve_prolong on cell-centred hierarchies with linear prolongation against the NumPy restatement
of tests/mgcl_cases.py.

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

import mg_restatement as rst
import mgcc_cases as cc
import mgcl_cases as cl
import mglines_cases as lc
from helpers import bits_equal, mismatch_report
from mg_restatement import EVEN, Halved, ODD

pytestmark = pytest.mark.gpu

ALL3, ALL2 = Halved((0, 1, 2)), Halved((0, 1))
MIX3 = [("dirichlet", "neumann"), ("neumann", "neumann"), ("neumann", "dirichlet")]
MIX2 = [("dirichlet", "neumann"), ("neumann", "dirichlet")]
FACE = {EVEN: "neumann", ODD: "dirichlet"}


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
    ns.lib.neptune_hip_init(0)
    ns.built = {name: form(steps, DAMP, dtype, faces) for name, (steps, faces, dtype, form) in PROBLEMS.items()}
    _prefetch(lowering, [t for _, texts, _ in ns.built.values() for t in texts])
    ns.entries = {}
    ns.cache = {}
    return ns


def _prefetch(lowering, texts):
    """every module compiled once, side by side (host threads only, nothing is loaded)"""
    from concurrent.futures import ThreadPoolExecutor

    def one(text):
        try:
            lowering.compile_module(text, load=False)
        except Exception:       # noqa: BLE001 - the test that needs this module shows the diagnostic
            pass
    with ThreadPoolExecutor(max_workers=12) as pool:
        list(pool.map(one, dict.fromkeys(texts)))


class Problem:
    pass


def _problem(nh, name):
    """the compiled operators, the restatement's levels, x0 and b: built once per problem, x0 and b left unchanged"""
    if name not in nh.cache:
        P = Problem()
        _, P.faces, P.dtype, _ = PROBLEMS[name]
        P.ref, P.texts, P.rests = nh.built[name]
        for t in P.texts:
            if t not in nh.entries:
                nh.entries[t] = nh.lowering.compile_module(t).geom_entry("entry")
        P.entries = [nh.entries[t] for t in P.texts]
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


def _hierarchy(nh, P, lines=None, constant=False):
    """a device hierarchy whose work fields hold NaN, every Linear pair of the restatement prolong="linear" with its faces
    (constant=True: none); -> (h, x, b)"""
    F = nh.fields.DeviceField
    levels = []
    for l, R in enumerate(P.ref):
        like = F.from_numpy(np.zeros(R.shape, P.dtype))
        bounds = ([s.start for s in R.where], [s.stop for s in R.where])
        others = [F.from_numpy(a) for a in P.rests[l]]
        stages = lines(l, P.entries[l], like, bounds, others) if lines else ()
        setting = {}
        if rst.axes_of(R).prolong == "linear" and not constant:
            setting = dict(prolong="linear", faces=[(FACE[lo], FACE[hi]) for lo, hi in R.axes.rim])
        levels.append(nh.mg.Level(P.entries[l], like, bounds, others=others, minv=F.from_numpy(R.minv), rscale=R.rscale, lines=stages,
                                  **setting))
    h = nh.mg.Hierarchy(levels)
    assert h.halved == [tuple(R.axes) if rst.axes_of(R).halved else () for R in P.ref[:-1]]
    assert [L.linear for L in h.levels[:-1]] == [rst.axes_of(R).prolong == "linear" and not constant for R in P.ref[:-1]]
    nan = lambda f: F.from_numpy(np.full(f.shape, np.nan, P.dtype))
    h.q = [nan(f) for f in h.q]
    h.x = [None] + [nan(f) for f in h.x[1:]]
    h.b = [None] + [nan(f) for f in h.b[1:]]
    return h, F.from_numpy(P.x0), F.from_numpy(P.b)


def _fields(h, x, b):
    return [x.numpy()] + [f.numpy() for f in h.x[1:]], [b.numpy()] + [f.numpy() for f in h.b[1:]]


def _solve(nh, P, max_cycles, tol2=0.0, check_every=1, constant=False):
    h, x, b = _hierarchy(nh, P, constant=constant)
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


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(8, 16, 264), (4, 8, 132), (2, 4, 66)] if name.startswith("3d") else
                                    [(16, 264), (8, 132), (4, 66)])
    assert all(L.axes.halved and L.axes.prolong == "linear" for L in P.ref[:-1])
    _check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_linear_on_the_first_pair_and_constant_on_the_second(nh):
    P = _problem(nh, "first_f64")
    assert [(rst.axes_of(L).kind, rst.axes_of(L).prolong, rst.axes_of(L).restrict) for L in P.ref[:-1]] == [("halved", "linear", "average"), ("halved", "constant", "average")]
    _check_against_reference(nh, P, 3)
    # and it is neither all-linear nor all-constant
    x_first = _reference(P, 3)[2][0]
    assert not bits_equal(x_first, _reference(_problem(nh, "2d_f64"), 3)[2][0])


def test_a_halved_plus_kept_pair(nh):
    P = _problem(nh, "kept_f64")
    assert [L.m for L in P.ref] == [(8, 264), (8, 132), (4, 66)] and [tuple(L.axes) for L in P.ref[:-1]] == [(1,), (0, 1)]
    _check_against_reference(nh, P, 3)


def test_linear_on_the_halved_pair_of_a_hierarchy_that_changes_its_grid_kind(nh):
    """Omega 14 -> 7 -> 3: the first pair halved and linear, the second vertex-centred"""
    P = _problem(nh, "switch_f64")
    assert [L.m for L in P.ref] == [(14, 14), (7, 7), (3, 3)] and [(rst.axes_of(L).kind, rst.axes_of(L).prolong, rst.axes_of(L).restrict) for L in P.ref[:-1]] == [("halved", "linear", "average"), ("coarsened", "constant", "average")]
    _check_against_reference(nh, P, 3)


@pytest.mark.parametrize("name", ["3d_f64", "3d_f32"])
def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch, name):
    P = _problem(nh, name)
    monkeypatch.delenv("NEPTUNE_HIP_MG_GRAPH", raising=False)
    res_g, xs_g, bs_g, counts_g = _solve(nh, P, 5)
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "0")          # read at every call
    res_p, xs_p, bs_p, counts_p = _solve(nh, P, 5)
    assert counts_g == (1, 4, 5) and counts_p == (5, 0, 5)
    assert res_g == res_p
    for a, b in zip(xs_g + bs_g, xs_p + bs_p):
        assert bits_equal(a, b), mismatch_report(a, b)
    assert bits_equal(xs_p[0], _reference(P, 5)[2][0])


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
    assert not bits_equal(ref[2][0], _reference(P, 4)[2][0])          # the stage changes the bits
    for graph in ("1", "0"):
        monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", graph)        # read at every call
        h, x, b = _hierarchy(nh, P, lines)
        assert h.has_lines and h.has_linear
        done, rr0, rr_last, rr_checks = nh.mg.solve(h, x, b, max_cycles=4)
        nh.torch.cuda.synchronize()
        assert done == 4 and nh.mg.counts() == ((1, 3, 4) if graph == "1" else (4, 0, 4))
        _compare(ref, rr0, rr_checks, *_fields(h, x, b))


def test_no_array_and_constant_everywhere_are_neptune_hip_mg_solve(nh):
    """prolong = NULL, and kind CONSTANT on every pair whatever the rules hold, give neptune_hip_mg_solve's bits, counts and
    scalars on a hierarchy of halved pairs"""
    P = _problem(nh, "3d_f64")
    (res, xs, bs, counts) = _solve(nh, P, 3, constant=True)
    for make in (lambda n: None, lambda n: (nh.capi.MgProlong * n)()):
        h, x, b = _hierarchy(nh, P, constant=True)
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
        for got, want in zip(sum(_fields(h, x, b), []), xs + bs):
            assert bits_equal(got, want), mismatch_report(got, want)
    # ... and these are not the linear solve's bits
    assert not bits_equal(xs[0], _reference(P, 3)[2][0])


def test_refusals_on_device_pointers_leave_every_field(nh):
    P = _problem(nh, "2d_f64")
    h, x, b = _hierarchy(nh, P)
    before = _fields(h, x, b)
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
    for got, want in zip(sum(_fields(h, x, b), []), sum(before, [])):
        assert bits_equal(got, want), mismatch_report(got, want)
    rc = nh.lib.neptune_hip_mg_solve_prolong(arr, None, prolong, len(h), h.dtype, 2, 2, 8, 2, 1, 0.0, None, None, None, None, None, None)
    nh.torch.cuda.synchronize()
    assert rc == nh.capi.OK
    assert bits_equal(x.numpy(), _reference(P, 2)[2][0])
    # a hierarchy with a linear pair is not for conjugate gradients
    with pytest.raises(ValueError, match="would not be a symmetric preconditioner"):
        nh.mg.cg_solve(h, x, b)


def test_stops_where_the_definition_says_and_before_constant_prolongation(nh):
    """32 x 32 x 32, Dirichlet faces, the threshold between cycles 5 and 6 of the linear sequence: the device stops at the
    restatement's expected_stop; with constant prolongation the same hierarchy has not got there two cycles later"""
    P = _problem(nh, "stop_f64")
    assert [L.m for L in P.ref] == [(32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3, (2,) * 3]
    seq = rst.rr_sequence(P.ref, P.x0, P.b, 7)
    tol2 = rst.tol_between(seq, 5, 6)
    max_cycles = len(seq) - 1
    want_done, want_checks = rst.expected_stop(seq, 1, max_cycles, tol2)
    assert want_done == 6
    (done, rr0, rr_last, rr_checks), _, _, counts = _solve(nh, P, max_cycles, tol2=tol2)
    print(f"seq = {seq}, tol2 = {tol2!r}, done = {done}, checks = {rr_checks}")
    assert (done, counts[2], len(rr_checks)) == (want_done, want_checks, want_checks)
    assert counts[0] + counts[1] == done
    assert rr_last == rr_checks[-1] <= tol2 and all(v > tol2 for v in rr_checks[:-1])
    (done_c, _, last_c, checks_c), _, _, _ = _solve(nh, P, want_done + 2, tol2=tol2, constant=True)
    print(f"constant: done = {done_c}, checks = {checks_c}")
    assert done_c == want_done + 2 > done and last_c > tol2
