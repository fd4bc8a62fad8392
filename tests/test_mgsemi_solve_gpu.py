"""neptune_hip_mg_solve and neptune_hip_mgcg_solve on semi-coarsened hierarchies against the NumPy restatement
of tests/mg_restatement.py, through the device harness of tests/mg_device.py.

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
import mg_device as mgd
import mg_restatement as rst
import mgsemi_cases as sc
from helpers import bits_equal

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


def _dots(name):
    """level 0 compiled with its dot entry: every problem MGCG runs on"""
    return () if name == "plan_f64" else (0,)


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"), check=("coarsened",))
    ns.built = {name: sc.build_levels(_steps(name), PROBLEMS[name][3], PROBLEMS[name][4]) for name in PROBLEMS}
    mgd.prefetch([(t, l in _dots(name)) for name, (_, texts) in ns.built.items() for l, t in enumerate(texts)])
    return ns


def _problem(nh, name):
    def build(P):
        P.dtype = PROBLEMS[name][4]
        P.ref, P.texts = nh.built[name]
        P.x0, P.b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype)
    return mgd.problem(nh, name, build, _dots(name))


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64", "3d_f32", "3d_f64"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(7, 15, 263), (7, 7, 131), (3, 3, 65), (3, 3, 32)] if name.startswith("3d") else
                                    [(15, 263), (7, 263), (7, 131), (3, 65)])
    mgd.check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    mgd.graph_vs_plain(nh, _problem(nh, "3d_f64"), monkeypatch, 5)


@pytest.mark.parametrize("check_every,between", [(1, (2, 3)), (3, (3, 6))])
def test_stops_where_the_definition_says_on_the_plan_hierarchy(nh, check_every, between):
    P = _problem(nh, "plan_f64")
    assert [L.m for L in P.ref[:5]] == [(63, 63), (63, 31), (63, 15), (63, 7), (31, 3)]
    mgd.check_stop(nh, P, check_every, between)


# ---------------------------------------------------------------- MGCG
@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", ["3d_f32", "3d_f64"])
def test_mgcg_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters):
    mgd.check_replay(nh, _problem(nh, name), iters, want_counts=(2, 0, 0, 2) if iters == 2 else (1, 4, 0, 5))


# ---------------------------------------------------------------- the Python wrappers
def test_python_wrappers(nh):
    P = _problem(nh, "3d_f64")
    h, x, b, _ = mgd.hierarchy(nh, P)
    assert h.coarsened == [(1, 2), (0, 1, 2), (2,)]
    for l, axes in enumerate(h.coarsened):
        assert nh.mg.coarsened_axes(h.levels[l], h.levels[l + 1]) == axes
        bounds = mgd.bounds(P.ref[l].where)
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
