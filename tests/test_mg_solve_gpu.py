"""neptune_hip_mg_solve: V-cycles whose fields never leave the device, against the NumPy restatement of
tests/mg_restatement.py.

No reduction enters a field, so after any number of cycles x_0 and every level's x_l, b_l must equal the restatement's bit
for bit, whatever the device's launch path (plain launches or the replayed graph of one cycle).  rr_0 and every rr read
after a block must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms.

Operator: mg_cases.mg_module, the unscaled Poisson star, one lowered module per level shape, rscale = 4; minv =
omega / (2 rank) on Omega and NaN outside; the work fields q_l and x_l, b_l (l >= 1) hold NaN before every call.

Stop: thresholds sit at the geometric mean of two consecutive check values of the restatement's r . r sequence, which the
test first requires to differ by a factor of 4 (tests/test_mg_host.py pins that the sequence falls that fast)."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_device as mgd
import mg_restatement as rst
import pcg_cases as pc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

# name: (Omega of level 0, levels, omega, dtype)
PROBLEMS = {
    "3d_f64": ((7, 15, 263), 3, 6.0 / 7.0, np.float64),
    "3d_f32": ((7, 15, 263), 3, 6.0 / 7.0, np.float32),
    "2d_f64": ((15, 263), 3, 0.8, np.float64),
}
PCG_OMEGA = (7, 15, 31)      # the two-input operator: two levels, 9 x 17 x 33 -> 5 x 9 x 17
BUILTIN_OMEGA = (7, 15, 31)


def _texts():
    out = {}
    for name, (omega, n_levels, _, dtype) in PROBLEMS.items():
        out[name] = [mgc.mg_module(shape, dtype) for shape, _ in mgc.level_shapes(omega, n_levels)]
    out["pcg"] = [pc.pcg_module(shape, np.float64) for shape, _ in mgc.level_shapes(PCG_OMEGA, 2)]
    out["builtin"] = [mgc.mg_module(shape, np.float64) for shape, _ in mgc.level_shapes(BUILTIN_OMEGA, 2)][1:]
    shape = mgc.level_shapes(PROBLEMS["3d_f64"][0], 1)[0][0]
    out["zero_diagonal"] = [mgc.mc.star_module(shape, np.float64, centre=0.0, side=1.0)]      # what jacobi_weights must refuse
    return out


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.texts = _texts()
    mgd.prefetch([(t, False) for ts in ns.texts.values() for t in ts])      # every module once, side by side
    return ns


def _problem(nh, name, rim=False):
    def build(P):
        omega, n_levels, damp, P.dtype = PROBLEMS[name]
        P.ref, P.texts = mgc.star_levels(omega, n_levels, P.dtype, damp, texts=nh.texts[name])
        P.x0, P.b = mgc.problem_fields(P.ref[0].shape, P.ref[0].where, P.dtype, rim=rim)
    return mgd.problem(nh, (name, rim), build)


@pytest.mark.parametrize("cycles", [2, 5])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_cycles_match_the_restatement(nh, name, cycles):
    P = _problem(nh, name)
    mgd.check_against_reference(nh, P, cycles, want_counts=(2, 0, 2) if cycles == 2 else (1, 4, 5))


def test_graph_and_plain_launches_give_identical_bits(nh, monkeypatch):
    mgd.graph_vs_plain(nh, _problem(nh, "3d_f64"), monkeypatch, 5)


@pytest.mark.parametrize("name,check_every,between", [("3d_f64", 1, (2, 3)), ("3d_f64", 3, (3, 6)), ("2d_f64", 3, (3, 6)),
                                                      ("3d_f32", 1, (1, 2))])
def test_stops_where_the_definition_says(nh, name, check_every, between):
    P = _problem(nh, name)
    mgd.check_stop(nh, P, check_every, between, cycles=6 if P.dtype == np.float64 else 3, label=f"{name}: ")


def test_a_converged_start_runs_no_cycle(nh):
    P = _problem(nh, "3d_f64")
    ref_rr0 = mgd.reference(P, 2)[0]
    (done, rr0, rr_last, rr_checks), xs, bs, counts = mgd.solve(nh, P, 5, tol2=2.0 * ref_rr0[0])
    assert (done, rr_checks, counts) == (0, [], (0, 0, 0))
    assert rr0 == rr_last and abs(rr0 - ref_rr0[0]) <= ref_rr0[1]
    assert bits_equal(xs[0], P.x0) and bits_equal(bs[0], P.b)
    # max_cycles = 0: rr_0 is still formed
    (done, rr0_again, _, rr_checks), xs, _, counts = mgd.solve(nh, P, 0)
    assert (done, rr_checks, counts, rr0_again) == (0, [], (0, 0, 0), rr0) and bits_equal(xs[0], P.x0)


def test_one_level_is_smoothing_only(nh):
    P = _problem(nh, "3d_f64")
    mgd.check_against_reference(nh, P, 2, n_levels=1, coarse_sweeps=3, want_counts=(2, 0, 2))
    mgd.check_against_reference(nh, P, 4, n_levels=1, coarse_sweeps=3, check_every=3, want_counts=(1, 3, 2))


def test_nonzero_dirichlet_rim(nh):
    P = _problem(nh, "3d_f64", rim=True)
    xs, _ = mgd.check_against_reference(nh, P, 2)
    outside = np.ones(P.x0.shape, bool)
    outside[P.ref[0].where] = False
    assert np.count_nonzero(P.x0[outside]) > 0 and bits_equal(xs[0][outside], P.x0[outside])
    zero = _problem(nh, "3d_f64")
    assert not bits_equal(xs[0], mgd.reference(zero, 2)[2][0])        # the rim values did enter, through A(x)


def test_two_input_operator_with_a_coefficient_per_level(nh):
    """pcg_cases.pcg_module on two levels, w injected to the coarse grid in numpy: in_rest per level"""
    def build(P):
        dtype = P.dtype = np.float64
        shapes = mgc.level_shapes(PCG_OMEGA, 2)
        P.texts = nh.texts["pcg"]
        w = [pc.w_field(shapes[0][0], dtype, values=(0.0, 1.0, 2.0, 4.0))]
        wc = np.zeros(shapes[1][0], dtype)
        wc[shapes[1][1]] = w[0][shapes[0][1]][1::2, 1::2, 1::2]     # the coarse cell j sits on the fine cell 2 j + 1
        w.append(wc)
        P.ref = []
        for text, (shape, where), wl in zip(P.texts, shapes, w):
            minv = np.full(shape, np.nan, dtype)
            minv[where] = (dtype(0.8) / (dtype(6.0) + wl[where])).astype(dtype)
            P.ref.append(rst.Level(rst.Operator(text, wl), shape, where, minv, dtype))
        P.rests = [[nh.fields.DeviceField.from_numpy(wl)] for wl in w]
        P.x0, P.b = mgc.problem_fields(shapes[0][0], shapes[0][1], dtype)
    P = mgd.problem(nh, "pcg", build)
    mgd.check_against_reference(nh, P, 3, want_counts=(1, 2, 3))
    rr0, checks, _, _ = mgd.reference(P, 3)
    assert checks[-1][0] < rr0[0]


def test_builtin_body_on_level_zero(nh):
    """level 0 runs the built-in 7-point body (fn = NULL), level 1 a lowered module"""
    dtype = np.float64
    shapes = mgc.level_shapes(BUILTIN_OMEGA, 2)
    P = mgd.Problem()
    P.dtype = dtype
    A0 = lambda u: helpers.oracle_entry("3d7", u)
    P.ref = [rst.Level(A0, shapes[0][0], shapes[0][1], mgc.minv_field(shapes[0][0], shapes[0][1], dtype, 0.125), dtype),
             rst.Level(rst.Operator(nh.texts["builtin"][0]), shapes[1][0], shapes[1][1],
                       mgc.minv_field(shapes[1][0], shapes[1][1], dtype, 0.8), dtype)]
    P.entries = [nh.capi.BODY_LAP3D7_F64, mgd.entry(nh, nh.texts["builtin"][0])]
    P.x0, P.b = mgc.problem_fields(shapes[0][0], shapes[0][1], dtype)
    mgd.check_against_reference(nh, mgd.finish(nh, P), 3, want_counts=(1, 2, 3))


def test_jacobi_weights(nh):
    P = _problem(nh, "3d_f64")
    R = P.ref[0]
    like = nh.fields.DeviceField.from_numpy(np.zeros(R.shape, P.dtype))
    bounds = ([s.start for s in R.where], [s.stop for s in R.where])
    diag = nh.apply.operator_diagonal(P.entries[0], like, bounds).numpy()
    outside = np.ones(R.shape, bool)
    outside[R.where] = False
    assert np.array_equal(diag[R.where], np.full(R.m, 6.0)) and not diag[outside].any()
    omega = 6.0 / 7.0
    w = nh.mg.jacobi_weights(P.entries[0], like, bounds, omega=omega).numpy()
    want = np.zeros(R.shape, P.dtype)
    want[R.where] = (np.float64(omega) / diag[R.where]).astype(P.dtype)
    assert bits_equal(w, want), mismatch_report(w, want)
    assert bits_equal(w[R.where], R.minv[R.where])
    # a zero diagonal is refused as apply.jacobi_minv refuses it
    zero = mgd.entry(nh, nh.texts["zero_diagonal"][0])
    with pytest.raises(ValueError, match="0 or not finite"):
        nh.mg.jacobi_weights(zero, like, bounds)
    # the Python layer names the level and the dimension of a hierarchy that does not nest
    L0 = nh.mg.Level(P.entries[0], like, bounds)
    with pytest.raises(ValueError, match="level 1, dimension 2"):
        nh.mg.Hierarchy([L0, nh.mg.Level(P.entries[1], nh.fields.DeviceField.from_numpy(np.zeros(P.ref[1].shape, P.dtype)),
                                         ([1, 1, 1], [4, 8, 131]))])


def test_refusals_on_device_pointers(nh):
    P = _problem(nh, "3d_f64")
    h, x, b, _ = mgd.hierarchy(nh, P)
    E, lib = nh.capi.EINVAL, nh.lib
    x.tensor.fill_(-3.0)

    def call(change=None, n_levels=3, dtype=nh.capi.F64, pre=2, post=2, coarse=8, max_cycles=4, check_every=1, stream=None):
        arr, keep = h._structs(x, b)
        if change:
            change(arr)
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        st = nh.fields.current_stream_ptr() if stream is None else stream
        rc = lib.neptune_hip_mg_solve(arr, n_levels, dtype, pre, post, coarse, max_cycles, check_every, 0.0, None, st, None,
                                      C.byref(done), C.byref(rr0), C.byref(last))
        return rc, done.value, rr0.value, last.value

    R = (E, 0, 0.0, 0.0)
    assert call(n_levels=0) == R and call(n_levels=17) == R and call(dtype=5) == R
    assert call(pre=-1) == R and call(post=-1) == R and call(coarse=-1) == R
    assert call(check_every=0) == R and call(max_cycles=-1) == R
    for field in ("x", "b", "q", "minv"):
        for level in range(3):
            assert call(lambda a: setattr(a[level], field, None)) == R, (field, level)
    fields = ("x", "b", "q", "minv")
    for i, fa in enumerate(fields):
        for fb in fields[i + 1:]:
            for level in range(3):
                assert call(lambda a: setattr(a[level], fa, getattr(a[level], fb))) == R, (fa, fb, level)
                n_bytes = int(np.prod(P.ref[level].shape)) * 8
                assert call(lambda a: setattr(a[level], fa, getattr(a[level], fb) + n_bytes - 8)) == R      # ... by one cell
        for fb in fields:
            assert call(lambda a: setattr(a[1], fa, getattr(a[0], fb))) == R, (fa, fb)
            assert call(lambda a: setattr(a[2], fa, getattr(a[1], fb) + 8)) == R, (fa, fb)

    def other_rank(a):
        a[2].g.rank = 2
    assert call(other_rank) == R

    def smaller_omega(d):
        def change(a):
            a[1].g.ub[d] -= 1
        return change
    for d in range(3):
        assert call(smaller_omega(d)) == R, d

    def empty(a):
        a[0].g.region_ub[0] = a[0].g.region_lb[0]
    assert call(empty) == R

    def shifted_input0(a):
        a[0].g.in_lb[0][0] += 1
        a[0].g.in_ub[0][0] += 1
    assert call(shifted_input0) == R
    for bad in (float("nan"), float("inf")):
        assert call(lambda a: setattr(a[1], "rscale", bad)) == R
    # a call while the stream is being captured: rr could not be read back
    torch = nh.torch
    side = torch.cuda.Stream()
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        scratch.add_(1.0)
        captured = call(stream=int(side.cuda_stream))
    assert captured == R
    torch.cuda.synchronize()
    assert bool((x.tensor == -3.0).all()) and bits_equal(b.numpy(), P.b)
    assert all(bool(nh.torch.isnan(f.tensor).all()) for f in h.q + h.x[1:] + h.b[1:])
    # rscale is unused on the last level: a NaN there is accepted
    assert call(lambda a: setattr(a[2], "rscale", float("nan")), max_cycles=1)[:2] == (nh.capi.OK, 1)
