"""neptune_hip_mgcg_solve_lines: conjugate gradients preconditioned with one line-smoothed V-cycle, against the
NumPy restatement of tests/mg_restatement.py.

The restatement's recurrences driven by the DEVICE's traced scalars (rz_0 and the rows pq_k, rz_(k+1), rr_(k+1)) must
reproduce x, r, p, z and every coarser level's x_l, b_l bit for bit, whatever the launch path (plain launches or the replayed
graph of one iteration).  Every traced scalar, rr_0 and rz_0 must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the
restatement's own terms.

Hierarchies: mg_cases' star operator on three levels 7 x 15 x 263 -> 3 x 7 x 131 -> 1 x 3 x 65 (f64 and f32) and on rank 2,
15 x 263 -> 7 x 131 -> 3 x 65, each under three configurations: (a) one stage along the contiguous dimension on every level;
(b) stages along every dimension in turn on level 0, one stage along dim 1 on level 1 and point Jacobi on level 2; (c) a
stage on level 1 only, so that level 0 takes the point-fused path of neptune_hip_mgcg_solve.  A level with stages is given no
minv.  The work fields hold NaN before every call.

Stop: on the 63 x 63 hierarchy of the flux-form operator with stages (0, 1) and V(1, 1), thresholds at the geometric mean of
two consecutive check values of the restatement's r . r sequence, which the test first requires to differ by a factor of 4."""
import ctypes as C

import numpy as np
import pytest

import mg_cases as mgc
import mg_device as mgd
import mg_restatement as rst
import mglines_cases as lc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

SHAPES = {"3d": ((7, 15, 263), 6.0 / 7.0), "2d": ((15, 263), 0.8)}
CONFIGS = {
    "3d": {"a": [(2,), (2,), (2,)], "b": [(0, 1, 2), (1,), ()], "c": [(), (1,), ()], "point": [(), (), ()]},
    "2d": {"a": [(1,), (1,), (1,)], "b": [(0, 1), (1,), ()], "c": [(), (1,), ()]},
}
# name: (shape key, dtype, configuration)
PROBLEMS = {f"{sk}_{tag}_{cfg}": (sk, dt, cfg)
            for sk, tag, dt in (("3d", "f64", np.float64), ("3d", "f32", np.float32), ("2d", "f64", np.float64)) for cfg in ("a", "b", "c")}
PROBLEMS["3d_f64_point"] = ("3d", np.float64, "point")


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.built, texts = {}, {}
    for name, (sk, dtype, cfg) in PROBLEMS.items():
        omega, damp = SHAPES[sk]
        key = (sk, np.dtype(dtype).name)
        levels, ts = lc.star_levels(omega, 3, dtype, damp, CONFIGS[sk][cfg], texts.get(key))
        texts[key] = ts
        if not levels[0].stages:       # the point-fused path forms z = minv_0 * r on the whole box
            levels[0].minv = mgc.minv_field(levels[0].shape, levels[0].where, dtype, damp, outside=0.0)
        ns.built[name] = (levels, ts)
    ns.flux = lc.flux_levels((0, 1))
    # every module once, side by side: level 0's with its dot entry
    mgd.prefetch([(t, l == 0) for ts in list(texts.values()) + [ns.flux[1]] for l, t in enumerate(ts)])
    return ns


def _problem(nh, name, rim=False):
    """the restatement's own stages on the device, and a level with stages gets no minv"""
    def build(P):
        if name == "flux":
            P.ref, P.texts, _ = nh.flux
            P.dtype = np.float64
            P.x0, P.b = lc.flux_problem(P.ref)
        else:
            P.dtype = PROBLEMS[name][1]
            P.ref, P.texts = nh.built[name]
            P.x0, P.b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype, rim=rim)
        P.rests = [R.A.rest for R in P.ref]
        P.lines = "stages"
    return mgd.problem(nh, (name, rim), build, dots=(0,))


def _bounds(R):
    return mgd.bounds(R.where)


def _solve(nh, P, max_iters, **kw):
    return mgd.cg(nh, P, max_iters, lines=True, **kw)


def _check_replay(nh, P, iters, **kw):
    """mg_device.check_replay through cg_solve(lines=True), and what the fields hold outside Omega"""
    return mgd.check_replay(nh, P, iters, outside=True, lines=True, **kw)


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("name", sorted(n for n in PROBLEMS if not n.endswith("point")))
def test_replay_from_the_traced_scalars_reproduces_every_field(nh, name, iters, sweeps):
    P = _problem(nh, name)
    sk, _, cfg = PROBLEMS[name]
    assert [L.m for L in P.ref] == ([(7, 15, 263), (3, 7, 131), (1, 3, 65)] if sk == "3d" else [(15, 263), (7, 131), (3, 65)])
    assert [tuple(s[0] for s in L.stages) for L in P.ref] == CONFIGS[sk][cfg]
    _check_replay(nh, P, iters, sweeps=sweeps, want_counts=(2, 0, 0, 2) if iters == 2 else (1, 4, 0, 5))


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    P = _problem(nh, "3d_f64_b")
    monkeypatch.delenv("NEPTUNE_HIP_MG_GRAPH", raising=False)
    G = _solve(nh, P, 5)
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "0")          # read at every call
    Pl = _check_replay(nh, P, 5, want_counts=(5, 0, 0, 5))
    assert G.counts == (1, 4, 0, 5)
    mgd.same_runs(G, Pl)


def test_fallback_runs_the_same_iteration(nh):
    """dot = "fallback": step 1 is a plain launch and neptune_hip_dot, the line stages unchanged"""
    _check_replay(nh, _problem(nh, "2d_f64_b"), 3, check_every=2, dot="fallback", want_counts=(1, 2, 3, 2))


def test_without_lines_it_is_mgcg_solve(nh):
    """lines = NULL, and n_stages = 0 on every level, against neptune_hip_mgcg_solve: the same bits, scalars and counts"""
    P = _problem(nh, "3d_f64_point")
    results = []
    for how in ("mgcg_solve", "null", "empty"):
        h, x, b, work = mgd.hierarchy(nh, P)
        arr, keep = h._structs(x, b)
        tr = nh.torch.zeros(15, dtype=nh.torch.float64, device="cuda")
        warr = (C.c_void_p * 3)(*[f.ptr for f in work])
        done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        fn_dot = C.cast(P.entries[0].fn_dot, C.c_void_p)
        rest = (fn_dot, 2, 8, warr, 5, 1, 0.0, tr.data_ptr(), None, None, C.byref(done), C.byref(rr0), C.byref(last))
        if how == "mgcg_solve":
            rc = nh.lib.neptune_hip_mgcg_solve(arr, 3, nh.capi.F64, *rest)
        else:
            lines = None if how == "null" else (nh.capi.MgLines * 3)()
            rc = nh.lib.neptune_hip_mgcg_solve_lines(arr, lines, 3, nh.capi.F64, *rest)
        nh.torch.cuda.synchronize()
        assert rc == nh.capi.OK
        results.append(((done.value, rr0.value, last.value, nh.mg.cg_counts(), nh.mg.cg_rz0()),
                        [tr.cpu().numpy(), x.numpy()] + [f.numpy() for f in work + h.x[1:] + h.b[1:]]))
    first = results[0]
    assert first[0][0] == 5 and first[0][3] == (1, 4, 0, 5)
    st, _, _, _, _ = rst.replay(P.ref, P.x0, P.b, first[0][4], first[1][0].reshape(-1, 3))
    x, r, p, z = st.x, st.r, st.p, st.z
    assert bits_equal(first[1][1], x) and bits_equal(first[1][4], z)
    for other in results[1:]:
        assert other[0] == first[0]
        for a, b in zip(other[1], first[1]):
            assert bits_equal(a, b), mismatch_report(a, b)


def test_nonzero_dirichlet_rim(nh):
    P = _problem(nh, "3d_f64_b", rim=True)
    R = _check_replay(nh, P, 2)
    outside = np.ones(P.x0.shape, bool)
    outside[P.ref[0].where] = False
    assert np.count_nonzero(P.x0[outside]) > 0 and bits_equal(R.x[outside], P.x0[outside])
    zero = _solve(nh, _problem(nh, "3d_f64_b"), 2)
    assert not bits_equal(R.x, zero.x)        # the rim values did enter, through A(x)


@pytest.mark.parametrize("check_every,between", [(1, (2, 3)), (3, (3, 6))])
def test_stops_where_the_definition_says_on_the_flux_hierarchy(nh, check_every, between):
    P = _problem(nh, "flux")
    assert [L.m for L in P.ref] == [(63, 63), (31, 31), (15, 15), (7, 7), (3, 3), (1, 1)]
    seq, tol2, max_iters, want = mgd.stop_schedule(P, lambda: rst.numpy_mgcg(P.ref, P.x0, P.b, 6, sweeps=1), check_every, between)
    R = _solve(nh, P, max_iters, tol2=tol2, check_every=check_every, trace=False, sweeps=1)
    mgd.check_cg_stop(R, seq, tol2, want)


def test_the_keyword_through_the_python_layer(nh):
    """Level(lines=...) from line_weights with no minv anywhere, cg_solve(lines=True) on it; without the keyword the hierarchy
    is still refused, and the message names the keyword; a hierarchy without stages runs the same either way"""
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
    with pytest.raises(ValueError, match="line stages.*lines=True"):
        nh.mg.cg_solve(h, x, b, max_iters=2)
    assert bits_equal(x.numpy(), P.x0)
    done, rr0, rr_last, trace = nh.mg.cg_solve(h, x, b, sweeps=1, max_iters=3, trace=True, lines=True)
    nh.torch.cuda.synchronize()
    want = rst.replay(P.ref, P.x0, P.b, nh.mg.cg_rz0(), trace, sweeps=1)[0].x
    assert done == 3 and bits_equal(x.numpy(), want), mismatch_report(x.numpy(), want)
    # no stages: the keyword changes nothing
    Q = _problem(nh, "3d_f64_point")
    runs = []
    for lines in (False, True):
        hq, xq, bq, work = mgd.hierarchy(nh, Q)
        res = nh.mg.cg_solve(hq, xq, bq, max_iters=3, trace=True, work=work, lines=lines)
        nh.torch.cuda.synchronize()
        runs.append((res[:3], res[3], xq.numpy()))
    assert runs[0][0] == runs[1][0] and bits_equal(runs[0][1], runs[1][1]) and bits_equal(runs[0][2], runs[1][2])
