"""neptune_hip_mg_solve and neptune_hip_mgcg_solve on semi-coarsened hierarchies against the NumPy restatement
of tests/mgsemi_cases.py.

No reduction enters a field, so after any number of cycles x_0 and every level's x_l, b_l must equal the restatement's bit
for bit, whatever the launch path (plain launches or the replayed graph of one cycle); for MGCG the restatement's recurrences
driven by the device's traced scalars must reproduce x, r, p, z and the coarser fields bit for bit.  rr_0, every rr read
after a block and every traced scalar must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms.

Hierarchies: rank 3, four levels 7 x 15 x 263 -> 7 x 7 x 131 -> 3 x 3 x 65 -> 3 x 3 x 32 (two axes, all axes, the contiguous
axis alone); rank 2, 15 x 263 -> 7 x 263 -> 7 x 131 -> 3 x 65 (the slow axis alone, the contiguous one alone, both).
Operators: mgcg_cases.aniso_module, one lowered module per level, the weights following the plan rule (w on a coarsened
dimension, 4 w on a kept one), rscale = 4; minv = damp / diagonal on Omega, +0 outside on level 0 (MGCG reads it there) and
NaN outside on the coarser levels; the work fields hold NaN before every call.

Stop: on the plan hierarchy of 63 x 63 with weights (0.03, 1), thresholds at the geometric mean of two consecutive check
values, which the test first requires to differ by a factor of 4 (tests/test_mgsemi_host.py pins that the sequence falls
that fast)."""
import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_restatement as rst
import mgsemi_cases as sc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

# name: (Omega of level 0, weights of level 0, the dimensions coarsened per pair (None: the plan rule), damp, dtype)
PROBLEMS = {
    "3d_f64": ((7, 15, 263), (0.03, 1.0, 1.0), [(1, 2), (0, 1, 2), (2,)], 6.0 / 7.0, np.float64),
    "3d_f32": ((7, 15, 263), (0.03, 1.0, 1.0), [(1, 2), (0, 1, 2), (2,)], 6.0 / 7.0, np.float32),
    "2d_f64": ((15, 263), (1.0, 0.25), [(0,), (1,), (0, 1)], 0.8, np.float64),
    "plan_f64": ((63, 63), (0.03, 1.0), None, 0.8, np.float64),
}


def _steps(name):
    omega, weights, axes, _, _ = PROBLEMS[name]
    return sc.plan(omega, weights) if axes is None else sc.with_axes(omega, weights, axes)


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
    ns.built = {name: sc.build_levels(_steps(name), PROBLEMS[name][3], PROBLEMS[name][4]) for name in PROBLEMS}
    _prefetch(lowering, [(t, l == 0 and name != "plan_f64") for name, (_, texts) in ns.built.items() for l, t in enumerate(texts)])
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
        P.dtype = PROBLEMS[name][4]
        P.ref, P.texts = nh.built[name]
        P.entries = [_entry(nh, t, l == 0 and name != "plan_f64") for l, t in enumerate(P.texts)]
        P.x0, P.b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype)
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


def _hierarchy(nh, P):
    """a device hierarchy whose work fields hold NaN; -> (h, x, b, [r, p, z])"""
    F = nh.fields.DeviceField
    levels = []
    for l, R in enumerate(P.ref):
        like = F.from_numpy(np.zeros(R.shape, P.dtype))
        bounds = ([s.start for s in R.where], [s.stop for s in R.where])
        levels.append(nh.mg.Level(P.entries[l], like, bounds, minv=F.from_numpy(R.minv), rscale=R.rscale))
    h = nh.mg.Hierarchy(levels)
    assert h.coarsened == [R.axes for R in P.ref[:-1]]
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
    assert [L.m for L in P.ref] == ([(7, 15, 263), (7, 7, 131), (3, 3, 65), (3, 3, 32)] if name.startswith("3d") else
                                    [(15, 263), (7, 263), (7, 131), (3, 65)])
    _check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


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
def test_stops_where_the_definition_says_on_the_plan_hierarchy(nh, check_every, between):
    P = _problem(nh, "plan_f64")
    assert [L.m for L in P.ref[:5]] == [(63, 63), (63, 31), (63, 15), (63, 7), (31, 3)]
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


# ---------------------------------------------------------------- MGCG
@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", ["3d_f32", "3d_f64"])
def test_mgcg_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    P = _problem(nh, name)
    h, x, b, work = _hierarchy(nh, P)
    done, rr0, rr_last, trace = nh.mg.cg_solve(h, x, b, max_iters=iters, trace=True, work=work)
    nh.torch.cuda.synchronize()
    counts, rz0 = nh.mg.cg_counts(), nh.mg.cg_rz0()
    assert done == iters and trace.shape == (iters, 3)
    assert counts == ((2, 0, 0, 2) if iters == 2 else (1, 4, 0, 5)), counts
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


# ---------------------------------------------------------------- the Python wrappers
def test_python_wrappers(nh):
    P = _problem(nh, "3d_f64")
    h, x, b, _ = _hierarchy(nh, P)
    assert h.coarsened == [(1, 2), (0, 1, 2), (2,)]
    for l, axes in enumerate(h.coarsened):
        assert nh.mg.coarsened_axes(h.levels[l], h.levels[l + 1]) == axes
        bounds = ([s.start for s in P.ref[l].where], [s.stop for s in P.ref[l].where])
        assert tuple(nh.mg.coarsen_bounds(bounds, axes=axes)) == P.ref[l + 1].m
    with pytest.raises(nh.capi.NeptuneHipError):
        nh.mg.coarsened_axes(h.levels[0], h.levels[0])
    with pytest.raises(nh.capi.NeptuneHipError):
        nh.mg.coarsened_axes(h.levels[0], h.levels[2])
    # restrict / prolong_add on a mixed pair of the hierarchy, as the solve launches them
    R0, R1 = P.ref[0], P.ref[1]
    F = nh.fields.DeviceField
    q = helpers.hash_field(R0.shape, P.dtype, seed=5)
    bc, xc = F.from_numpy(np.full(R1.shape, np.nan)), F.from_numpy(np.full(R1.shape, np.nan))
    nh.mg.restrict(h.levels[0], h.levels[1], b, F.from_numpy(q), bc, xc)
    want_b, want_x = rst.restrict(P.b, q, R0.where, R0.rscale, np.full(R1.shape, np.nan), np.full(R1.shape, np.nan), R1.where, R0.axes)
    nh.torch.cuda.synchronize()
    assert bits_equal(bc.numpy(), want_b) and bits_equal(xc.numpy(), want_x)
    xf = F.from_numpy(q)
    nh.mg.prolong_add(h.levels[0], h.levels[1], bc, xf)
    nh.torch.cuda.synchronize()
    assert bits_equal(xf.numpy(), rst.prolong_add(want_b, R1.where, q, R0.where, R0.axes))
    # a hierarchy from coarsening_plan is the restated one
    plan = nh.mg.coarsening_plan((63, 63), (0.03, 1.0))
    assert [(p[0], p[2]) for p in plan] == [(L.m, L.axes) for L in _problem(nh, "plan_f64").ref]
