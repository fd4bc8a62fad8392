"""neptune_hip_mg_solve_lines and the Python layer around it against the NumPy restatement of
tests/mg_restatement.py.

No reduction enters a field, so after any number of cycles x_0 and every level's x_l, b_l must equal the restatement's bit
for bit, whatever the launch path (plain launches or the replayed graph of one cycle); rr_0 and every rr read after a block
must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms (the bounds of test_mg_solve_gpu.py).

Hierarchies: mg_cases' star operator on three levels 7 x 15 x 263 -> 3 x 7 x 131 -> 1 x 3 x 65 (f64 and f32) and on rank 2,
15 x 263 -> 7 x 131 -> 3 x 65, each under two configurations: (a) one stage along the contiguous dimension on every level;
(b) stages along every dimension in turn on level 0, one stage along dim 1 on level 1 and point Jacobi on level 2.  A level
with stages is given no minv.  The work fields hold NaN before every call.

Stop: on the 63 x 63 hierarchy of the flux-form operator with alternating stages, thresholds at the geometric mean of two
consecutive check values, which the test first requires to differ by a factor of 4 (tests/test_mglines_host.py pins that
the sequence falls that fast)."""
import ctypes as C

import numpy as np
import pytest

import mg_cases as mgc
import mg_device as mgd
import mg_restatement as rst
import mglines_cases as lc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

# name: (Omega of level 0, damp, dtype, the stages' axes per level)
PROBLEMS = {
    "3d_f64_a": ((7, 15, 263), 6.0 / 7.0, np.float64, [(2,), (2,), (2,)]),
    "3d_f64_b": ((7, 15, 263), 6.0 / 7.0, np.float64, [(0, 1, 2), (1,), ()]),
    "3d_f32_a": ((7, 15, 263), 6.0 / 7.0, np.float32, [(2,), (2,), (2,)]),
    "3d_f32_b": ((7, 15, 263), 6.0 / 7.0, np.float32, [(0, 1, 2), (1,), ()]),
    "2d_f64_a": ((15, 263), 0.8, np.float64, [(1,), (1,), (1,)]),
    "2d_f64_b": ((15, 263), 0.8, np.float64, [(0, 1), (1,), ()]),
    "3d_f64_point": ((7, 15, 263), 6.0 / 7.0, np.float64, [(), (), ()]),
}


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.built = {}
    texts = {}
    for name, (omega, damp, dtype, axes) in PROBLEMS.items():
        key = (omega, np.dtype(dtype).name)
        ns.built[name] = lc.star_levels(omega, 3, dtype, damp, axes, texts.get(key))
        texts[key] = ns.built[name][1]
    ns.flux = lc.flux_levels((0, 1))
    ns.flux32 = lc.flux_levels((0, 1), n=17, dtype=np.float32)
    mgd.prefetch([(t, False) for t in [t for _, ts in ns.built.values() for t in ts] + ns.flux[1] + ns.flux32[1]])
    return ns


def _problem(nh, name):
    """the restatement's own stages on the device, and a level with stages gets no minv"""
    def build(P):
        if name == "flux":
            P.ref, P.texts, _ = nh.flux
            P.dtype = np.float64
            P.x0, P.b = lc.flux_problem(P.ref)
        else:
            P.dtype = PROBLEMS[name][2]
            P.ref, P.texts = nh.built[name]
            P.x0, P.b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype)
        P.rests = [R.A.rest for R in P.ref]
        P.lines = "stages"
    return mgd.problem(nh, name, build)


def _bounds(R):
    return mgd.bounds(R.where)


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", ["2d_f64_a", "2d_f64_b", "3d_f32_a", "3d_f32_b", "3d_f64_a", "3d_f64_b"])
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    assert [L.m for L in P.ref] == ([(7, 15, 263), (3, 7, 131), (1, 3, 65)] if name.startswith("3d") else [(15, 263), (7, 131), (3, 65)])
    assert [tuple(s[0] for s in L.stages) for L in P.ref] == PROBLEMS[name][3]
    mgd.check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    mgd.graph_vs_plain(nh, _problem(nh, "3d_f64_b"), monkeypatch, 5)


def test_without_lines_it_is_mg_solve(nh):
    """lines = NULL, and n_stages = 0 on every level, against neptune_hip_mg_solve: the same bits, rr values and counts"""
    P = _problem(nh, "3d_f64_point")
    results = []
    for how in ("mg_solve", "null", "empty"):
        h, x, b, _ = mgd.hierarchy(nh, P)
        arr, keep = h._structs(x, b)
        rr = (C.c_double * 5)()
        done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        rest = (2, 2, 8, 5, 1, 0.0, rr, None, None, C.byref(done), C.byref(rr0), C.byref(last))
        if how == "mg_solve":
            rc = nh.lib.neptune_hip_mg_solve(arr, 3, nh.capi.F64, *rest)
        else:
            lines = None if how == "null" else (nh.capi.MgLines * 3)()
            rc = nh.lib.neptune_hip_mg_solve_lines(arr, lines, 3, nh.capi.F64, *rest)
        nh.torch.cuda.synchronize()
        assert rc == nh.capi.OK
        results.append((done.value, rr0.value, last.value, list(rr), nh.mg.counts(), x.numpy(), [f.numpy() for f in h.x[1:] + h.b[1:]]))
    first = results[0]
    assert first[0] == 5 and first[4] == (1, 4, 5)
    _, _, ref_x, _ = mgd.reference(P, 5)
    assert bits_equal(first[5], ref_x[0])
    for other in results[1:]:
        assert other[:5] == first[:5]
        assert bits_equal(other[5], first[5])
        for a, b in zip(other[6], first[6]):
            assert bits_equal(a, b)


@pytest.mark.parametrize("check_every,between", [(1, (2, 3)), (3, (3, 6))])
def test_stops_where_the_definition_says_on_the_flux_hierarchy(nh, check_every, between):
    P = _problem(nh, "flux")
    assert [L.m for L in P.ref] == [(63, 63), (31, 31), (15, 15), (7, 7), (3, 3), (1, 1)]
    mgd.check_stop(nh, P, check_every, between)


# ---------------------------------------------------------------- the Python layer
def _flux_level(nh, built, l):
    levels, texts, coefs = built
    F = nh.fields.DeviceField
    R = levels[l]
    like = F.from_numpy(np.zeros(R.shape, R.dt))
    return R, like, [F.from_numpy(a) for a in coefs[l]], mgd.entry(nh, texts[l])


@pytest.mark.parametrize("l", [0, 3, 5])
def test_operator_tridiagonal_on_the_flux_operator(nh, l):
    """against the entries computed from a and c in NumPy, bit for bit: 63 x 63, 7 x 7 and the one-cell level"""
    R, like, others, entry = _flux_level(nh, nh.flux, l)
    a, c = (f.numpy() for f in others)
    for axis in (0, 1):
        got = nh.mg.operator_tridiagonal(entry, like, _bounds(R), axis, others)
        want = lc.flux_tridiagonal(a, c, axis)
        for name, g, w in zip(("lower", "diag", "upper"), got, want):
            assert bits_equal(g.numpy(), w), f"{name} along {axis}: " + mismatch_report(g.numpy(), w)
    with pytest.raises(ValueError, match="reach along axis"):
        nh.mg.operator_tridiagonal(entry, like, _bounds(R), 0, others, reach=[0, 1])
    with pytest.raises(ValueError, match="outside"):
        nh.mg.operator_tridiagonal(entry, like, _bounds(R), 2, others)


@pytest.mark.parametrize("which", ["f64", "f32"])
def test_line_weights_match_the_restatement(nh, which):
    built, l = (nh.flux, 1) if which == "f64" else (nh.flux32, 0)
    R, like, others, entry = _flux_level(nh, built, l)
    for axis in (0, 1):
        stage = nh.mg.line_weights(entry, like, _bounds(R), axis, others, omega=lc.FLUX_DAMP)
        ax, lo, inv, up = R.stages[axis]
        assert stage.axis == ax == axis
        for name, g, w in zip(("lo", "inv", "up"), (stage.lo, stage.inv, stage.up), (lo, inv, up)):
            w = np.where(np.isnan(w), 0, w).astype(w.dtype)           # the restatement's levels carry NaN outside Omega; the definition +0
            assert bits_equal(g.numpy(), w), f"{name} along {axis}: " + mismatch_report(g.numpy(), w)
    with pytest.raises(ValueError, match="pivots"):
        nh.mg.line_weights(entry, like, _bounds(R), 0, others, omega=0.0)        # T / 0: no finite pivot


def test_levels_with_lines_through_the_python_layer(nh):
    """Level(lines=...) from line_weights, line_smooth on it, solve through neptune_hip_mg_solve_lines, cg_solve's refusal"""
    P = _problem(nh, "flux")
    F = nh.fields.DeviceField
    levels = []
    for l, R in enumerate(P.ref):
        like = F.from_numpy(np.zeros(R.shape, P.dtype))
        others = [F.from_numpy(a) for a in R.A.rest]
        lines = [nh.mg.line_weights(P.entries[l], like, _bounds(R), ax, others, omega=lc.FLUX_DAMP) for ax in (0, 1)]
        levels.append(nh.mg.Level(P.entries[l], like, _bounds(R), others=others, rscale=R.rscale, lines=lines))
    h = nh.mg.Hierarchy(levels)
    assert h.has_lines and all(L.minv is None for L in h.levels)
    x, b = F.from_numpy(P.x0), F.from_numpy(P.b)
    done, rr0, rr_last, rr_checks = nh.mg.solve(h, x, b, max_cycles=3)
    nh.torch.cuda.synchronize()
    _, _, ref_x, _ = mgd.reference(P, 3)
    assert done == 3 and bits_equal(x.numpy(), ref_x[0]), mismatch_report(x.numpy(), ref_x[0])
    with pytest.raises(ValueError, match="line stages"):
        nh.mg.cg_solve(h, x, b, max_iters=2)
    # line_smooth alone on level 0: one stage from q = A(x)
    R = P.ref[0]
    q = R.A(P.b)
    xd, qd = F.from_numpy(P.b), F.from_numpy(q)
    nh.mg.line_smooth(h.levels[0], h.levels[0].lines[1], qd, b, xd)
    nh.torch.cuda.synchronize()
    ax, lo, inv, up = R.stages[1]
    want = rst.line_stage(q, P.b, lo, inv, up, P.b, R.where, ax)
    assert bits_equal(xd.numpy(), want), mismatch_report(xd.numpy(), want)
    # a hierarchy without stages still needs minv, and says so
    bare = nh.mg.Hierarchy([nh.mg.Level(P.entries[0], levels[0].like, _bounds(R), others=levels[0].others)])
    with pytest.raises(ValueError, match="no minv"):
        nh.mg.solve(bare, x, b, max_cycles=1)
