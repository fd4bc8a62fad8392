"""neptune_hip_mg_solve, neptune_hip_mgcg_solve and their line-stage and mixed-precision forms on cell-centred hierarchies
 against the NumPy restatement of tests/mg_restatement.py.

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
    ns.built = {name: cc.flux_levels(steps, DAMP, dtype, faces) for name, (steps, faces, dtype) in PROBLEMS.items()}
    _prefetch(lowering, [(t, l == 0 and name in DOT) for name, (_, texts, _) in ns.built.items() for l, t in enumerate(texts)])
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
        _, P.faces, P.dtype = PROBLEMS[name]
        P.ref, P.texts, P.rests = nh.built[name]
        P.entries = [_entry(nh, t, l == 0 and name in DOT) for l, t in enumerate(P.texts)]
        P.x0, b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype)
        P.b = cc.compatible(b, P.ref[0].where) if P.faces == "neumann" else b
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


def _levels(nh, P, lines=None):
    F = nh.fields.DeviceField
    levels = []
    for l, R in enumerate(P.ref):
        like = F.from_numpy(np.zeros(R.shape, P.dtype))
        bounds = ([s.start for s in R.where], [s.stop for s in R.where])
        others = [F.from_numpy(a) for a in P.rests[l]]
        stages = lines(l, P.entries[l], like, bounds, others) if lines else ()
        levels.append(nh.mg.Level(P.entries[l], like, bounds, others=others, minv=F.from_numpy(R.minv), rscale=R.rscale, lines=stages))
    return levels


def _hierarchy(nh, P, lines=None):
    """a device hierarchy whose work fields hold NaN; -> (h, x, b, [r, p, z])"""
    F = nh.fields.DeviceField
    h = nh.mg.Hierarchy(_levels(nh, P, lines))
    assert h.coarsened == [tuple(R.axes) for R in P.ref[:-1]]
    assert h.halved == [tuple(R.axes) if rst.axes_of(R).halved else () for R in P.ref[:-1]]
    nan = lambda f: F.from_numpy(np.full(f.shape, np.nan, P.dtype))
    h.q = [nan(f) for f in h.q]
    h.x = [None] + [nan(f) for f in h.x[1:]]
    h.b = [None] + [nan(f) for f in h.b[1:]]
    return h, F.from_numpy(P.x0), F.from_numpy(P.b), [nan(h.q[0]) for _ in range(3)]


def _solve(nh, P, max_cycles, tol2=0.0, check_every=1):
    h, x, b, _ = _hierarchy(nh, P)
    res = nh.mg.solve(h, x, b, max_cycles=max_cycles, tol2=tol2, check_every=check_every)
    nh.torch.cuda.synchronize()
    xs = [x.numpy()] + [f.numpy() for f in h.x[1:]]
    bs = [b.numpy()] + [f.numpy() for f in h.b[1:]]
    return res, xs, bs, nh.mg.counts()


def _check_against_reference(nh, P, cycles, check_every=1, want_counts=None):
    (done, rr0, rr_last, rr_checks), xs, bs, counts = _solve(nh, P, cycles, check_every=check_every)
    ref_rr0, ref_checks, ref_x, ref_b = _reference(P, cycles, check_every)
    assert done == cycles and len(rr_checks) == len(ref_checks) == -(-cycles // check_every)
    if want_counts is not None:
        assert counts == want_counts, counts
    print(f"rr0 = {rr0!r} (terms' sum {ref_rr0[0]!r}, bound {ref_rr0[1]:.3e})")
    assert abs(rr0 - ref_rr0[0]) <= ref_rr0[1]
    for k, (got, (want, bound)) in enumerate(zip(rr_checks, ref_checks)):
        print(f"  check {k}: rr = {got!r} (terms' sum {want!r}, bound {bound:.3e})")
        assert abs(got - want) <= bound
    assert rr_last == rr_checks[-1]
    for l, (got, want) in enumerate(zip(xs, ref_x)):
        assert bits_equal(got, want), f"x_{l}: " + mismatch_report(got, want)
    for l, (got, want) in enumerate(zip(bs, ref_b)):
        assert bits_equal(got, want), f"b_{l}: " + mismatch_report(got, want)


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(8, 16, 264), (4, 8, 132), (2, 4, 66)] if name.startswith("3d") else
                                    [(16, 264), (8, 132), (4, 66)])
    _check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_a_halved_plus_kept_pair(nh):
    P = _problem(nh, "kept_f64")
    assert [L.m for L in P.ref] == [(8, 264), (8, 132), (4, 66)] and [L.weights for L in P.ref] == [(1.0, 1.0), (4.0, 1.0), (4.0, 1.0)]
    _check_against_reference(nh, P, 3)


def test_a_hierarchy_that_changes_its_grid_kind(nh):
    """the first pair halved, the second vertex-centred: Omega 14 -> 7 -> 3"""
    P = _problem(nh, "switch_f64")
    assert [L.m for L in P.ref] == [(14, 14), (7, 7), (3, 3)]
    h, _, _, _ = _hierarchy(nh, P)
    assert h.halved == [(0, 1), ()] and h.coarsened == [(0, 1), (0, 1)]
    _check_against_reference(nh, P, 3)


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    P = _problem(nh, "3d_f64")
    monkeypatch.delenv("NEPTUNE_HIP_MG_GRAPH", raising=False)
    res_g, xs_g, bs_g, counts_g = _solve(nh, P, 5)
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "0")          # read at every call
    res_p, xs_p, bs_p, counts_p = _solve(nh, P, 5)
    assert counts_g == (1, 4, 5) and counts_p == (5, 0, 5)
    assert res_g == res_p
    for a, b in zip(xs_g + bs_g, xs_p + bs_p):
        assert bits_equal(a, b), mismatch_report(a, b)
    _, _, ref_x, _ = _reference(P, 5)
    assert bits_equal(xs_p[0], ref_x[0])


@pytest.mark.parametrize("check_every,between", [(1, (2, 3)), (3, (3, 6))])
def test_stops_where_the_definition_says(nh, check_every, between):
    P = _problem(nh, "stop_f64")
    assert [L.m for L in P.ref] == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    if "seq" not in P.runs:
        P.runs["seq"] = rst.rr_sequence(P.ref, P.x0, P.b, 6)
    seq = P.runs["seq"]
    tol2 = rst.tol_between(seq, *between)
    max_cycles = len(seq) - 1
    want_done, want_checks = rst.expected_stop(seq, check_every, max_cycles, tol2)
    assert want_done == between[1]
    (done, rr0, rr_last, rr_checks), _, _, counts = _solve(nh, P, max_cycles, tol2=tol2, check_every=check_every)
    print(f"seq = {seq}, tol2 = {tol2!r}, done = {done}, checks = {rr_checks}")
    assert (done, counts[2], len(rr_checks)) == (want_done, want_checks, want_checks)
    assert counts[0] + counts[1] == done
    assert rr_last == rr_checks[-1] <= tol2 and all(v > tol2 for v in rr_checks[:-1])


# ---------------------------------------------------------------- MGCG on the Neumann operator
@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", ["3d_f32", "3d_f64"])
def test_mgcg_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    P = _problem(nh, name)
    h, x, b, work = _hierarchy(nh, P)
    done, rr0, rr_last, trace = nh.mg.cg_solve(h, x, b, max_iters=iters, trace=True, work=work)
    nh.torch.cuda.synchronize()
    counts, rz0 = nh.mg.cg_counts(), nh.mg.cg_rz0()
    assert done == iters and trace.shape == (iters, 3)
    # counts[2], how many iterations took a plain launch and a separate dot product, is the operator's matter: the
    # dot-monitored launch may refuse this many-input apply, and the replay from the traced scalars holds either way
    print(f"counts = {counts}")
    assert (counts[0], counts[1], counts[3]) == ((2, 0, 2) if iters == 2 else (1, 4, 5)), counts
    st, checks, rr0_ref, rz0_ref, _ = rst.replay(P.ref, P.x0, P.b, rz0, trace)
    rx, rr, rp, rz = st.x, st.r, st.p, st.z
    print(f"rr0 = {rr0!r} (terms' sum {rr0_ref[0]!r}, bound {rr0_ref[1]:.3e})  rz0 = {rz0!r} (sum {rz0_ref[0]!r}, bound {rz0_ref[1]:.3e})")
    assert abs(rr0 - rr0_ref[0]) <= rr0_ref[1] and abs(rz0 - rz0_ref[0]) <= rz0_ref[1]
    for k, sums in enumerate(checks):
        print(f"  k={k}: " + "  ".join(f"{nm} = {trace[k][c]!r} (sum {s!r}, bound {bd:.3e})"
                                        for c, (nm, (s, bd)) in enumerate(zip(("pq", "rz'", "rr'"), sums))))
        for c, (s, bd) in enumerate(sums):
            assert abs(float(trace[k][c]) - s) <= bd
    assert rr_last == float(trace[-1][2])
    for nm, got, want in (("x", x.numpy(), rx), ("r", work[0].numpy(), rr), ("p", work[1].numpy(), rp), ("z", work[2].numpy(), rz)):
        assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)
    for l in range(1, len(P.ref)):
        got, want = h.x[l].numpy(), P.ref[l].x
        assert bits_equal(got, want), f"x_{l}: " + mismatch_report(got, want)
        got, want = h.b[l].numpy(), P.ref[l].b
        assert bits_equal(got, want), f"b_{l}: " + mismatch_report(got, want)


def _cg_sequence(P):
    """r . r of the restatement's recurrences (numpy's own sums) down to 1e-16 rr_0, computed once: -> (seq, tol2)"""
    if "cg_seq" not in P.runs:
        rr0 = rst.numpy_mgcg(P.ref, P.x0, P.b, 0)[0]
        P.runs["cg_seq"] = (rst.numpy_mgcg(P.ref, P.x0, P.b, 20, stop_at=1e-16 * rr0), 1e-16 * rr0)
    return P.runs["cg_seq"]


def test_mgcg_iteration_count_on_the_neumann_operator(nh):
    """to 1e-16 rr_0: the count of the restatement's recurrences, whose r . r at the stop and one iteration before must be a
    factor of 2 either side of the threshold, so that the count cannot hinge on a summation order"""
    P = _problem(nh, "cg_f64")
    assert [L.m for L in P.ref] == [(8, 8, 32), (4, 4, 16), (2, 2, 8), (2, 2, 4), (2, 2, 2)]
    seq, tol2 = _cg_sequence(P)
    n = len(seq) - 1
    print(f"seq = {seq}, tol2 = {tol2!r}")
    assert 1 <= n < 20 and seq[n] <= 0.5 * tol2 and seq[n - 1] >= 2.0 * tol2, "precondition on the restatement"
    h, x, b, work = _hierarchy(nh, P)
    done, rr0, rr_last = nh.mg.cg_solve(h, x, b, max_iters=20, tol2=tol2, work=work)
    nh.torch.cuda.synchronize()
    print(f"done = {done}, rr0 = {rr0!r}, rr_last = {rr_last!r}")
    assert done == n and rr_last <= tol2 < rr0
    assert np.isfinite(x.numpy()).all()


def test_mixed_precision_smoke(nh):
    """f64 conjugate gradients on the Neumann operator around the f32 cycle of the same hierarchy: it reaches 1e-16 rr_0 in
    about the iterations of the f64 solver"""
    P64, P32 = _problem(nh, "cg_f64"), _problem(nh, "cg_f32")
    seq, tol2 = _cg_sequence(P64)
    F = nh.fields.DeviceField
    outer = _levels(nh, P64)[0]
    inner = nh.mg.Hierarchy(_levels(nh, P32))
    assert inner.halved == [(0, 1, 2), (0, 1, 2), (2,), (2,)]
    x, b = F.from_numpy(P64.x0), F.from_numpy(P64.b)
    work = [F.from_numpy(np.full(P64.x0.shape, np.nan)) for _ in range(3)]
    nan32 = lambda f: F.from_numpy(np.full(f.shape, np.nan, np.float32))
    inner.q = [nan32(f) for f in inner.q]
    inner.x = [nan32(inner.q[0])] + [nan32(f) for f in inner.x[1:]]
    inner.b = [nan32(inner.q[0])] + [nan32(f) for f in inner.b[1:]]
    done, rr0, rr_last, trace = nh.mg.cg_solve_mixed(outer, inner, x, b, max_iters=20, tol2=tol2, trace=True, work=work)
    nh.torch.cuda.synchronize()
    rz0 = nh.mg.cg_rz0()
    print(f"mixed: done = {done} (f64: {len(seq) - 1}), rr0 = {rr0!r}, rr_last = {rr_last!r}")
    assert 1 <= done <= len(seq) + 1 and rr_last <= tol2 < rr0 and np.isfinite(x.numpy()).all()
    # every field against the composed restatement, driven by the device's scalars: f64 recurrences on the f64 operator
    # around the f32 cycle of the halved hierarchy
    R = mx.Problem(P64.ref[0].A, P32.ref)
    st, sums, rr0_ref, rz0_ref, _ = rst.replay(R, P64.x0, P64.b, rz0, trace)
    assert trace.shape == (done, 3) and abs(rr0 - rr0_ref[0]) <= rr0_ref[1] and abs(rz0 - rz0_ref[0]) <= rz0_ref[1]
    for k, row in enumerate(sums):
        for c, (s, bd) in enumerate(row):
            assert abs(float(trace[k][c]) - s) <= bd, (k, c, trace[k][c], s, bd)
    for nm, got, want in (("x", x.numpy(), st.x), ("r", work[0].numpy(), st.r), ("p", work[1].numpy(), st.p),
                          ("r32", inner.b[0].numpy(), st.r32), ("z32", inner.x[0].numpy(), st.z32)):
        assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)
    for l in range(1, len(P32.ref)):
        for nm, got, want in ((f"x_{l}", inner.x[l].numpy(), P32.ref[l].x), (f"b_{l}", inner.b[l].numpy(), P32.ref[l].b)):
            assert bits_equal(got, want), f"{nm}: " + mismatch_report(got, want)


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
        ref_x, ref_b = [L.x.copy() for L in P.ref], [L.b.copy() for L in P.ref]
    finally:
        del R1.stages
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", graph)        # read at every call
        h, x, b, _ = _hierarchy(nh, P, lines)
        assert h.has_lines
        for nm, got, want in zip(("lo", "inv", "up"), h.levels[1].lines[0][1:], stage[1:]):
            assert bits_equal(got.numpy(), want), f"line_weights' {nm}: " + mismatch_report(got.numpy(), want)
        done, rr0, rr_last, rr_checks = nh.mg.solve(h, x, b, max_cycles=4)
        nh.torch.cuda.synchronize()
        print(f"graph = {graph}: rr0 = {rr0!r}, checks = {rr_checks}, counts = {nh.mg.counts()}")
        assert done == 4 and all(after < 0.5 * before for before, after in zip([rr0] + rr_checks, rr_checks))
        out.append(x.numpy())
        assert abs(rr0 - ref_rr0[0]) <= ref_rr0[1]
        for got, (want, bound) in zip(rr_checks, ref_checks):
            assert abs(got - want) <= bound
        for l, (got, want) in enumerate(zip([x.numpy()] + [f.numpy() for f in h.x[1:]], ref_x)):
            assert bits_equal(got, want), f"x_{l}: " + mismatch_report(got, want)
        for l, (got, want) in enumerate(zip([b.numpy()] + [f.numpy() for f in h.b[1:]], ref_b)):
            assert bits_equal(got, want), f"b_{l}: " + mismatch_report(got, want)
    assert bits_equal(out[0], out[1]), mismatch_report(out[0], out[1])
