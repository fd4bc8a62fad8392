"""neptune_hip_mg_solve, neptune_hip_mgcg_solve and their line-stage and mixed-precision forms on cell-centred hierarchies
 against the NumPy restatement of tests/mg_restatement.py, through the device harness of tests/mg_device.py.

No reduction enters a field, so after any number of cycles x_0 and every level's x_l, b_l must equal the restatement's bit
for bit, whatever the launch path (plain launches or the replayed graph of one cycle); for MGCG the restatement's recurrences
driven by the device's traced scalars must reproduce x, r, p, z and the coarser fields bit for bit.  rr_0, every rr read
after a block and every traced scalar must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms.

Operators: mgcc_cases.flux_module, one lowered module per level, with face coefficients that vanish on the boundary faces
(Neumann) and, for Dirichlet faces, a diagonal field; rscale = 4, minv = 0.8 / diagonal on Omega, +0 outside on level 0 (MGCG
reads it there) and NaN outside on the coarser levels; the work fields hold NaN before every call.  The right-hand side of a
Neumann problem is made compatible (its mean over Omega taken off).

Hierarchies: rank 3, f64 and f32, 8 x 16 x 264 -> 4 x 8 x 132 -> 2 x 4 x 66 with Neumann faces; rank 2, 16 x 264 -> 8 x 132 ->
4 x 66 with Dirichlet faces; a halved-plus-kept pair, 8 x 264 -> 8 x 132 -> 4 x 66; a hierarchy that changes its grid kind,
14 x 14 -> 7 x 7 (halved) -> 3 x 3 (vertex-centred).  Stop: the plan hierarchy of 32 x 32 with Dirichlet faces, thresholds
at the geometric mean of two consecutive check values, which the test first requires to differ by a factor of 4
(tests/test_mgcc_host.py pins that the sequence falls that fast).  Iteration count of MGCG: the plan hierarchy of 8 x 8 x 32
with Neumann faces, five levels down to 2 x 2 x 2 with kept dimensions on the way -- the three-level hierarchy above leaves a
2 x 4 x 66 Neumann level to 8 Jacobi sweeps and serves for bits only."""
import numpy as np
import pytest

import mg_cases as mgc
import mg_device as mgd
import mg_restatement as rst
import mgcc_cases as cc
import mgcgmixed_cases as mx
import mglines_cases as lc
from helpers import bits_equal, mismatch_report
from mg_restatement import Halved

pytestmark = pytest.mark.gpu

ALL3, ALL2 = Halved((0, 1, 2)), Halved((0, 1))
# name: (the steps [(extents, weights, axes)], faces, dtype)
PROBLEMS = {
    "3d_f64": (cc.halved_steps((8, 16, 264), [ALL3, ALL3]), "neumann", np.float64),
    "3d_f32": (cc.halved_steps((8, 16, 264), [ALL3, ALL3]), "neumann", np.float32),
    "2d_f64": (cc.halved_steps((16, 264), [ALL2, ALL2]), "dirichlet", np.float64),
    "kept_f64": (cc.halved_steps((8, 264), [Halved((1,)), ALL2]), "dirichlet", np.float64),
    "switch_f64": (cc.halved_steps((14, 14), [ALL2, (0, 1)]), "dirichlet", np.float64),
    "stop_f64": (cc.plan((32, 32)), "dirichlet", np.float64),
    "cg_f64": (cc.plan((8, 8, 32)), "neumann", np.float64),
    "cg_f32": (cc.plan((8, 8, 32)), "neumann", np.float32),
}
DOT = ("3d_f64", "3d_f32", "cg_f64")        # level 0 compiled with its dot entry: the problems MGCG runs on
DAMP = 0.8


def _dots(name):
    return (0,) if name in DOT else ()


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"), check=("coarsened", "halved"))
    ns.built = {name: cc.flux_levels(steps, DAMP, dtype, faces) for name, (steps, faces, dtype) in PROBLEMS.items()}
    mgd.prefetch([(t, l in _dots(name)) for name, (_, texts, _) in ns.built.items() for l, t in enumerate(texts)])
    return ns


def _problem(nh, name):
    def build(P):
        _, P.faces, P.dtype = PROBLEMS[name]
        P.ref, P.texts, P.rests = nh.built[name]
        P.x0, b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype)
        P.b = cc.compatible(b, P.ref[0].where) if P.faces == "neumann" else b
    return mgd.problem(nh, name, build, _dots(name))


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(8, 16, 264), (4, 8, 132), (2, 4, 66)] if name.startswith("3d") else
                                    [(16, 264), (8, 132), (4, 66)])
    mgd.check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_a_halved_plus_kept_pair(nh):
    P = _problem(nh, "kept_f64")
    assert [L.m for L in P.ref] == [(8, 264), (8, 132), (4, 66)] and [L.weights for L in P.ref] == [(1.0, 1.0), (4.0, 1.0), (4.0, 1.0)]
    mgd.check_against_reference(nh, P, 3)


def test_a_hierarchy_that_changes_its_grid_kind(nh):
    """the first pair halved, the second vertex-centred: Omega 14 -> 7 -> 3"""
    P = _problem(nh, "switch_f64")
    assert [L.m for L in P.ref] == [(14, 14), (7, 7), (3, 3)]
    h, _, _, _ = mgd.hierarchy(nh, P)
    assert h.halved == [(0, 1), ()] and h.coarsened == [(0, 1), (0, 1)]
    mgd.check_against_reference(nh, P, 3)


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    mgd.graph_vs_plain(nh, _problem(nh, "3d_f64"), monkeypatch, 5)


@pytest.mark.parametrize("check_every,between", [(1, (2, 3)), (3, (3, 6))])
def test_stops_where_the_definition_says(nh, check_every, between):
    P = _problem(nh, "stop_f64")
    assert [L.m for L in P.ref] == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    mgd.check_stop(nh, P, check_every, between)


# ---------------------------------------------------------------- MGCG on the Neumann operator
@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", ["3d_f32", "3d_f64"])
def test_mgcg_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    mgd.check_replay(nh, _problem(nh, name), iters, want_counts=(2, 0, 2) if iters == 2 else (1, 4, 5), any_fallback=True)


def test_mgcg_iteration_count_on_the_neumann_operator(nh):
    """to 1e-16 rr_0: the count of the restatement's recurrences (mg_device.check_iteration_count)"""
    P = _problem(nh, "cg_f64")
    assert [L.m for L in P.ref] == [(8, 8, 32), (4, 4, 16), (2, 2, 8), (2, 2, 4), (2, 2, 2)]
    _, _, _, x = mgd.check_iteration_count(nh, P, 20)
    assert np.isfinite(x).all()


def test_mixed_precision_smoke(nh):
    """f64 conjugate gradients on the Neumann operator around the f32 cycle of the same hierarchy: it reaches 1e-16 rr_0 in
    about the iterations of the f64 solver"""
    P64, P32 = _problem(nh, "cg_f64"), _problem(nh, "cg_f32")
    seq, tol2 = mgd.cg_sequence(P64, 20)
    outer, inner, x, b, work = mgd.mixed(nh, P64, P32)
    assert inner.halved == [(0, 1, 2), (0, 1, 2), (2,), (2,)]
    done, rr0, rr_last, trace = nh.mg.cg_solve_mixed(outer, inner, x, b, max_iters=20, tol2=tol2, trace=True, work=work)
    nh.torch.cuda.synchronize()
    rz0 = nh.mg.cg_rz0()
    print(f"mixed: done = {done} (f64: {len(seq) - 1}), rr0 = {rr0!r}, rr_last = {rr_last!r}")
    assert 1 <= done <= len(seq) + 1 and rr_last <= tol2 < rr0 and np.isfinite(x.numpy()).all()
    # every field against the composed restatement, driven by the device's scalars: f64 recurrences on the f64 operator
    # around the f32 cycle of the halved hierarchy
    R = mx.Problem(P64.ref[0].A, P32.ref)
    st, sums, rr0_ref, rz0_ref, _ = rst.replay(R, P64.x0, P64.b, rz0, trace)
    assert trace.shape == (done, 3)
    mgd.check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, sums)
    for nm, got, want in (("x", x.numpy(), st.x), ("r", work[0].numpy(), st.r), ("p", work[1].numpy(), st.p),
                          ("r32", inner.b[0].numpy(), st.r32), ("z32", inner.x[0].numpy(), st.z32)):
        mgd.same(nm, got, want)
    mgd.check_levels(*[[f.numpy() for f in fs[1:]] for fs in (inner.x, inner.b)], P32.ref)


def test_a_line_stage_on_level_one_smoke(nh, monkeypatch):
    """solve() with a line stage along the contiguous dimension on level 1 of the Dirichlet hierarchy: the line-stage driver
    takes the halved pairs through the same cycle code; r . r falls at every check and both launch paths give the same bits"""
    P = _problem(nh, "2d_f64")

    def lines(l, entry, like, bounds, others):
        return [nh.mg.line_weights(entry, like, bounds, axis=1, others=others, omega=DAMP, reach=1)] if l == 1 else ()
    # the reference: the composed restatement on the same levels, level 1 with the stage's factors from the operator's own
    # coefficient fields (the boundary faces' coefficients are 0: no coupling leaves Omega)
    R1, (c0, c1, _) = P.ref[1], P.rests[1]
    up_coef = np.zeros_like(c1)
    up_coef[:, :-1] = c1[:, 1:]
    diag = cc.face_fields(R1.m, P.dtype, P.faces, R1.weights)[1]
    stage = (1,) + lc.factors(-c1, diag, -up_coef, R1.where, 1, DAMP)
    R1.stages = [stage]
    try:
        ref_rr0, ref_checks = rst.run(P.ref, P.x0, P.b, 4)
        ref = (ref_rr0, ref_checks, [L.x.copy() for L in P.ref], [L.b.copy() for L in P.ref])
    finally:
        del R1.stages
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", graph)        # read at every call
        h, x, b, _ = mgd.hierarchy(nh, P, lines=lines)
        assert h.has_lines
        for nm, got, want in zip(("lo", "inv", "up"), h.levels[1].lines[0][1:], stage[1:]):
            assert bits_equal(got.numpy(), want), f"line_weights' {nm}: " + mismatch_report(got.numpy(), want)
        done, rr0, rr_last, rr_checks = nh.mg.solve(h, x, b, max_cycles=4)
        nh.torch.cuda.synchronize()
        print(f"graph = {graph}: rr0 = {rr0!r}, checks = {rr_checks}, counts = {nh.mg.counts()}")
        assert done == 4 and all(after < 0.5 * before for before, after in zip([rr0] + rr_checks, rr_checks))
        out.append(x.numpy())
        mgd.compare(ref, rr0, rr_checks, *mgd.fields_of(h, x, b))
    assert bits_equal(out[0], out[1]), mismatch_report(out[0], out[1])
