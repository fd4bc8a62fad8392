"""The linear prolongation on cell-centred pairs without a GPU: the two new exports against the header, every
refusal on host pointers (the argument checks run before the device is touched), the restatement's prolongation as dense
matrices, the Python layer's errors, and the convergence the GPU tests and DESIGN's table rely on -- conditions on the
restatement (tests/mg_restatement.py), not on the code under test.  On the parent commit the library lacks both exports, so the
fixture fails and with it every test that takes it."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_restatement as rst
import mgcc_cases as cc
import mgcl_cases as cl
from mg_restatement import EVEN, Halved, Linear, ODD
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    lib = _capi.load()
    assert hasattr(lib, "neptune_hip_mg_prolong_add_linear") and hasattr(lib, "neptune_hip_mg_solve_prolong")
    return lib


def _geom(omega, lo=None):
    lo = [1] * len(omega) if lo is None else list(lo)
    box = ([0] * len(omega), [l + m + 1 for l, m in zip(lo, omega)])
    return make_geom(box, (lo, [l + m for l, m in zip(lo, omega)]))


def _prolong(kind, lo=(0, 0, 0), hi=(0, 0, 0)):
    p = _capi.MgProlong()
    p.kind = kind
    for d in range(3):
        p.rim_lo[d], p.rim_hi[d] = lo[d], hi[d]
    return p


# ---------------------------------------------------------------- exports and prototypes
def test_exports_and_prototypes_match_the_header(lib):
    header = " ".join(_capi.HEADER_PATH.read_text().split())
    for text in ("#define NEPTUNE_HIP_MG_PROLONG_CONSTANT 0", "#define NEPTUNE_HIP_MG_PROLONG_LINEAR 1",
                 "#define NEPTUNE_HIP_MG_RIM_EVEN 0", "#define NEPTUNE_HIP_MG_RIM_ODD 1",
                 "typedef struct { int32_t kind; int32_t rim_lo[3], rim_hi[3]; } neptune_hip_mg_prolong_t;",
                 "int neptune_hip_mg_prolong_add_linear(int dtype, const neptune_hip_apply_geom_t *g_fine, const "
                 "neptune_hip_apply_geom_t *g_coarse, const neptune_hip_mg_prolong_t *p, const void *x_coarse, void *x_fine, "
                 "void *stream);",
                 "int neptune_hip_mg_solve_prolong(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, "
                 "const neptune_hip_mg_prolong_t *prolong, int n_levels, int dtype, int pre, int post, int coarse_sweeps, "
                 "int64_t max_cycles, int64_t check_every, double tol2, double *rr_checks, void *stream, const "
                 "neptune_hip_launch_cfg_t *cfg, int64_t *cycles_done, double *rr0, double *rr_last);",
                 "p = 0.75 * e[j]; s = 0.25 * v; t = p + s"):
        assert text in header, text
    assert (_capi.MG_PROLONG_CONSTANT, _capi.MG_PROLONG_LINEAR, _capi.MG_RIM_EVEN, _capi.MG_RIM_ODD) == (0, 1, 0, 1) == (0, 1, EVEN, ODD)
    assert C.sizeof(_capi.MgProlong) == 28 and [f[0] for f in _capi.MgProlong._fields_] == ["kind", "rim_lo", "rim_hi"]
    restype, args = _capi.SIGNATURES["neptune_hip_mg_prolong_add_linear"]
    assert restype is C.c_int and len(args) == 7 and args[3] is C.POINTER(_capi.MgProlong)
    restype, args = _capi.SIGNATURES["neptune_hip_mg_solve_prolong"]
    lines = _capi.SIGNATURES["neptune_hip_mg_solve_lines"][1]
    assert restype is C.c_int and args[:2] == lines[:2] and args[2] is C.POINTER(_capi.MgProlong) and args[3:] == lines[2:]


# ---------------------------------------------------------------- refusals on host pointers: nothing may be launched
def test_the_kernel_entry_refuses_on_host_pointers(lib):
    xc, xf = np.full((5, 9, 17), 5.0), np.full((8, 16, 32), 3.0)
    gf, gc = _geom((6, 14, 30)), _geom((3, 7, 15))
    E, f64 = _capi.EINVAL, _capi.F64

    def call(p, g_fine=gf, g_coarse=gc, coarse=xc, fine=xf, dtype=f64):
        return lib.neptune_hip_mg_prolong_add_linear(dtype, C.byref(g_fine), C.byref(g_coarse), C.byref(p) if p is not None else None,
                                                     coarse.ctypes.data, fine.ctypes.data, None)
    lin = _capi.MG_PROLONG_LINEAR
    assert call(None) == E
    assert call(_prolong(2)) == E and call(_prolong(-1)) == E                          # a kind outside {0, 1}
    for d in range(3):                                                                 # a rule outside {0, 1}, per face
        for bad in (2, -1):
            lo, hi = [0, 1, 0], [1, 0, 1]
            lo[d] = bad
            assert call(_prolong(lin, lo=lo, hi=[1, 0, 1])) == E, (d, bad)
            hi[d] = bad
            assert call(_prolong(lin, lo=[0, 1, 0], hi=hi)) == E, (d, bad)
    # ... also on a dimension the pair keeps (dimension 0 here): it is a dimension < rank of a LINEAR pair
    assert call(_prolong(lin, lo=(7, 0, 0)), g_coarse=_geom((6, 7, 15))) == E
    # LINEAR on a pair with no halved dimension: a vertex-centred one
    assert call(_prolong(lin), g_fine=_geom((7, 15, 31))) == E
    # what neptune_hip_mg_prolong_add refuses, for either kind
    for p in (_prolong(lin), _prolong(_capi.MG_PROLONG_CONSTANT)):
        assert call(p, g_fine=_geom((6, 15, 30))) == E                                 # halved and coarsened in one pair
        assert call(p, g_fine=gc, g_coarse=gc) == E                                    # all kept
        assert call(p, g_coarse=_geom((3, 7, 14))) == E                                # dimension 2 in no state
        assert call(p, g_coarse=_geom((7, 15))) == E                                   # ranks differ
        assert call(p, coarse=xf) == E                                                 # x_fine overlaps x_coarse
        assert call(p, dtype=7) == E
    assert (xc == 5.0).all() and (xf == 3.0).all()


def _solve_args(omegas, body=_capi.BODY_LAP3D7_F64):
    arrays = [[np.full(tuple(m + 2 for m in om), 1.5) for _ in range(4)] for om in omegas]
    levels = (_capi.MgLevel * len(omegas))()
    for l, om in enumerate(omegas):
        L = levels[l]
        L.fn, L.body, L.g = None, body, _geom(om)
        L.x, L.b, L.q, L.minv = (a.ctypes.data for a in arrays[l])
        L.rscale = 4.0
    return levels, arrays


def test_the_solve_refuses_on_host_pointers(lib):
    lin, const = _capi.MG_PROLONG_LINEAR, _capi.MG_PROLONG_CONSTANT

    def solve(omegas, prolong, n_levels=None, max_cycles=4, check_every=1, pre=2, lines=None, body=_capi.BODY_LAP3D7_F64):
        levels, arrays = _solve_args(omegas, body)
        arr = None
        if prolong is not None:
            arr = (_capi.MgProlong * len(prolong))(*prolong)
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mg_solve_prolong(levels, lines, arr, len(omegas) if n_levels is None else n_levels, _capi.F64, pre, 2, 8,
                                              max_cycles, check_every, 0.0, None, None, None, C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        assert all((a == 1.5).all() for level in arrays for a in level), "a refusal leaves every field's bits unchanged"
        return rc
    E = _capi.EINVAL
    good = [(8, 16, 32), (4, 8, 16), (2, 4, 8)]
    ok = [_prolong(lin, (1, 1, 1), (1, 1, 1)), _prolong(lin)]
    # the new refusals, on either pair
    for l in range(2):
        for bad in (_prolong(2), _prolong(-3), _prolong(lin, lo=(0, 2, 0)), _prolong(lin, hi=(0, 0, -1))):
            prolong = list(ok)
            prolong[l] = bad
            assert solve(good, prolong) == E, (l, bad.kind)
    assert solve([(8, 16, 32), (8, 8, 16), (4, 4, 8)], [_prolong(lin, lo=(5, 0, 0)), _prolong(lin)]) == E     # on a kept dimension
    assert solve([(7, 15, 31), (3, 7, 15)], [_prolong(lin)]) == E                      # LINEAR on a vertex-centred pair
    assert solve([(14, 14, 14), (7, 7, 7), (3, 3, 3)], [_prolong(lin), _prolong(lin)]) == E       # ... on the second pair only
    # every existing refusal of neptune_hip_mg_solve_lines, with the array present
    assert solve([(8, 15, 32), (4, 7, 16)], [_prolong(lin)]) == E                      # a mixed pair
    assert solve([(8, 16, 32), (8, 16, 32)], [_prolong(const)]) == E                   # all kept
    assert solve(good, ok, n_levels=0) == E and solve(good, ok, n_levels=17) == E
    assert solve(good, ok, max_cycles=-1) == E and solve(good, ok, check_every=0) == E and solve(good, ok, pre=-1) == E
    assert solve(good, ok, body=_capi.BODY_LAP3D27_F32) == E                           # a built-in body of another element type
    stages = (_capi.MgLines * 3)()
    stages[1].n_stages = 4
    assert solve(good, ok, lines=stages) == E
    stages[1].n_stages = 1
    stages[1].axis[0] = 3
    assert solve(good, ok, lines=stages) == E
    # entries of dimensions >= rank and the rules of a CONSTANT pair are not read: these reach the device, which the host
    # test cannot follow -- test_mgcl_solve_gpu.py runs them


# ---------------------------------------------------------------- the prolongation as dense matrices
def _line_P(n, rule_lo, rule_hi):
    axes = Linear((0,), ((rule_lo, rule_hi),))
    return cc.dense(lambda e: rst.prolong_add(e, (slice(0, n // 2),), np.zeros(n), (slice(0, n),), axes), n // 2, n)


@pytest.mark.parametrize("rule_lo,rule_hi", [(EVEN, EVEN), (ODD, ODD), (EVEN, ODD), (ODD, EVEN)])
def test_dense_matrix_on_an_8_to_16_line(rule_lo, rule_hi):
    P = _line_P(16, rule_lo, rule_hi)
    assert P.shape == (16, 8)
    want = np.zeros((16, 8))
    for i in range(1, 15):                                     # interior rows: (1/4, 3/4) for even i, (3/4, 1/4) for odd i
        j = i // 2
        want[i, j] = 0.75
        want[i, j + 1 if i % 2 else j - 1] = 0.25
    want[0, 0] = 1.0 if rule_lo == EVEN else 0.5               # the ghost folds onto the edge cell: 3/4 +- 1/4
    want[15, 7] = 1.0 if rule_hi == EVEN else 0.5
    assert np.array_equal(P, want)
    sums = P @ np.ones(8)
    assert np.array_equal(sums[1:15], np.ones(14))
    assert sums[0] == (1.0 if rule_lo == EVEN else 0.5) and sums[15] == (1.0 if rule_hi == EVEN else 0.5)
    if (rule_lo, rule_hi) == (EVEN, EVEN):
        assert np.array_equal(sums, np.ones(16))               # constants are reproduced exactly on every cell
    # a linear function's coarse samples (cell centres 2 j + 1 in fine half-cells ...) give the fine cell-centre values
    coarse = 3.0 + 0.5 * (2.0 * np.arange(8) + 1.0)            # u(s) = 3 + s / 2 at the coarse centres s = 2 j + 1 (fine cell widths)
    fine = 3.0 + 0.5 * (np.arange(16) + 0.5)                   # ... and at the fine centres s = i + 1/2
    assert np.array_equal((P @ coarse)[1:15], fine[1:15])
    # ODD: a function that is odd about the face, u = s, is reproduced on the edge row too
    if rule_lo == ODD:
        assert (P @ (2.0 * np.arange(8) + 1.0))[0] == 0.5
    # P is not a multiple of the averaging restriction's transpose: the cycle is not a symmetric preconditioner
    R = cc.dense(lambda e: rst.restrict(e, np.zeros(16), (slice(0, 16),), 1.0, np.zeros(8), np.zeros(8), (slice(0, 8),), Halved((0,)))[0],
                 16, 8)
    assert not np.array_equal(P, 2.0 * R.T)


def test_a_one_cell_coarse_line_has_two_ghosts():
    for rule_lo, rule_hi, want in ((EVEN, EVEN, [1.0, 1.0]), (ODD, ODD, [0.5, 0.5]), (EVEN, ODD, [1.0, 0.5]), (ODD, EVEN, [0.5, 1.0])):
        assert np.array_equal(_line_P(2, rule_lo, rule_hi), np.array(want).reshape(2, 1))


def test_tensor_product_against_einsum_on_dyadic_data():
    """rank 3, dimensions 0 and 2 halved, 1 kept, Omega inside boxes with unequal rims holding NaN outside the coarse Omega:
    the restatement is the tensor product of the line matrices -- exactly, on data whose products and sums are exact"""
    fm, cm = (4, 3, 8), (2, 3, 4)
    fshape, cshape = (6, 6, 11), (5, 4, 6)
    fw = tuple(slice(l, l + m) for l, m in zip((1, 2, 3), fm))
    cw = tuple(slice(l, l + m) for l, m in zip((2, 1, 1), cm))
    rim = ((ODD, EVEN), (ODD, ODD), (EVEN, ODD))
    rng = np.random.default_rng(11)
    e = np.full(cshape, np.nan)
    e[cw] = rng.integers(-64, 64, cm) / 8.0                    # dyadic: every product with 3/4, 1/4 and every sum is exact
    x_f = np.full(fshape, 7.0)
    got = rst.prolong_add(e, cw, x_f, fw, Linear((0, 2), rim))
    P0, P2 = _line_P(4, *rim[0]), _line_P(8, *rim[2])
    assert np.array_equal(got[fw], 7.0 + np.einsum("ia,kc,ajc->ijk", P0, P2, e[cw]))
    outside = np.ones(fshape, bool)
    outside[fw] = False
    assert (got[outside] == 7.0).all() and (x_f == 7.0).all()
    # the ghost of the later dimension is +- the INTERMEDIATE at the edge: the corner cell's weight is the product of the two
    # edge rows, (3/4 - 1/4) (3/4 - 1/4) = 1/4 for two ODD faces
    one = np.zeros((2, 2))
    one[0, 0] = 1.0
    corner = rst.prolong_add(one, (slice(0, 2),) * 2, np.zeros((4, 4)), (slice(0, 4),) * 2, Linear((0, 1), ((ODD, EVEN), (ODD, EVEN))))
    assert corner[0, 0] == 0.25 and corner[0, 1] == 0.5 * 0.75 and corner[1, 1] == 0.75 * 0.75 and corner[3, 3] == 0.0


def test_the_dispatch_of_the_restatement():
    """a Linear marker goes to the linear prolongation and to mgcc_cases' averaging restriction; anything else is mgcc_cases'"""
    d = helpers.hash_field((14,), np.float64, seed=5)
    w14, w7 = (slice(0, 14),), (slice(0, 7),)
    lin = Linear((0,), ((EVEN, ODD),))
    assert lin.halved and lin == (0,) and lin.rim == ((EVEN, ODD),)
    b7, _ = rst.restrict(d, np.zeros(14), w14, 1.0, np.zeros(7), np.zeros(7), w7, lin)
    assert np.array_equal(b7, 0.5 * (d[0::2] + d[1::2]))
    assert np.array_equal(rst.prolong_add(b7, w7, np.zeros(14), w14, Halved((0,))), np.repeat(b7, 2))
    got = rst.prolong_add(b7, w7, np.zeros(14), w14, lin)
    assert got[0] == 0.75 * b7[0] + 0.25 * b7[0] and got[13] == 0.75 * b7[6] + 0.25 * -b7[6]
    assert got[5] == 0.75 * b7[2] + 0.25 * b7[3] and got[6] == 0.75 * b7[3] + 0.25 * b7[2]


def test_the_two_input_form_of_the_operator_is_the_flux_form():
    """mgcl_cases.star_s_module with s = +1 per Dirichlet and -1 per Neumann boundary face against mgcc_cases' flux form with
    unit coefficients, on fields that vanish outside Omega: the same operator (to rounding: the terms are added in another
    order) and the same smoother weights"""
    faces = [("dirichlet", "neumann"), ("neumann", "neumann"), ("neumann", "dirichlet")]
    steps = cc.halved_steps((4, 6, 8), [Halved((0, 1, 2))])
    star, _, _ = cl.star_levels(steps, 0.8, np.float64, faces)
    flux, _, _ = cl.flux_levels(steps, 0.8, np.float64, faces)
    for S, Fl in zip(star, flux):
        u = np.zeros(S.shape)
        u[S.where] = helpers.hash_field(S.m, np.float64, seed=9)
        assert np.allclose(S.A(u)[S.where], Fl.A(u)[Fl.where], rtol=0, atol=1e-14)
        assert np.array_equal(S.minv[S.where], Fl.minv[Fl.where])


# ---------------------------------------------------------------- the Python layer
class _Like:
    """what Level and Hierarchy read of a field before anything is allocated"""

    def __init__(self, shape):
        self.shape, self.rank, self.dtype = tuple(shape), len(shape), _capi.F64
        self.lb, self.box = [0] * len(shape), ([0] * len(shape), list(shape))


@pytest.fixture()
def no_device_fields(monkeypatch):
    from neptune_hip import multigrid
    monkeypatch.setattr(multigrid.DeviceField, "empty_like", staticmethod(lambda like: None))


def _hierarchy(omegas, settings):
    from neptune_hip import multigrid
    return multigrid.Hierarchy([multigrid.Level(None, _Like([m + 2 for m in om]), ([1] * len(om), [m + 1 for m in om]), **kw)
                                for om, kw in zip(omegas, settings)])


def test_level_settings_reach_the_c_structs(no_device_fields):
    lin = dict(prolong="linear")
    h = _hierarchy([(8, 16, 32), (4, 8, 16), (2, 8, 8), (1, 4, 4)],
                   [dict(faces="dirichlet", **lin), {}, dict(faces=[("neumann", "dirichlet"), ("dirichlet", "dirichlet"), ("neumann", "neumann")], **lin),
                    dict(prolong="linear")])               # the last level's setting is ignored, faces missing or not
    assert h.has_linear and [L.linear for L in h.levels] == [True, False, True, True]
    arr = h._prolong_structs()
    assert len(arr) == 3
    assert [(p.kind, list(p.rim_lo), list(p.rim_hi)) for p in arr] == [(1, [1, 1, 1], [1, 1, 1]), (0, [0, 0, 0], [0, 0, 0]),
                                                                       (1, [0, 1, 0], [1, 1, 0])]
    assert not _hierarchy([(8, 16), (4, 8)], [{}, dict(prolong="linear")]).has_linear
    h2 = _hierarchy([(8, 16), (4, 8)], [dict(prolong="linear", faces="neumann"), {}])
    assert [(p.kind, list(p.rim_lo), list(p.rim_hi)) for p in h2._prolong_structs()] == [(1, [0, 0, 0], [0, 0, 0])]


def test_hierarchy_names_the_level_of_a_bad_setting(no_device_fields):
    good = [(8, 16), (4, 8), (2, 4)]
    with pytest.raises(ValueError, match=r'level 1: prolong="linear" needs faces'):
        _hierarchy(good, [{}, dict(prolong="linear"), {}])
    for faces in ("periodic", ("neumann", "dirichlet"), [("neumann", "dirichlet")], [("neumann",), ("neumann", "neumann")],
                  [("neumann", "open"), ("neumann", "neumann")], 3, [(0, 1), (1, 0)]):
        with pytest.raises(ValueError, match=r"level 0: faces is .* not "):
            _hierarchy(good, [dict(prolong="linear", faces=faces), {}, {}])
    with pytest.raises(ValueError, match=r'level 1: prolong is "constant" or "linear", not \'cubic\''):
        _hierarchy(good, [{}, dict(prolong="cubic"), {}])
    # "linear" on a level whose pair below has no halved dimension: a vertex-centred pair
    with pytest.raises(ValueError, match=r'level 1: prolong="linear" needs a cell-centred pair, but no dimension is halved towards level 2'):
        _hierarchy([(14, 14), (7, 7), (3, 3)], [dict(prolong="linear", faces="dirichlet"), dict(prolong="linear", faces="dirichlet"), {}])
    _hierarchy([(14, 14), (7, 7), (3, 3)], [dict(prolong="linear", faces="dirichlet"), {}, {}])
    _hierarchy(good, [dict(faces="nonsense"), {}, {}])       # faces without "linear" is not looked at: defaults change nothing


def test_cg_solve_refuses_a_linear_pair(no_device_fields):
    from neptune_hip import multigrid
    h = _hierarchy([(8, 16), (4, 8)], [dict(prolong="linear", faces="dirichlet"), {}])

    class _Field:
        box, dtype = h.levels[0].like.box, _capi.F64
    with pytest.raises(ValueError, match="would not be a symmetric preconditioner"):
        multigrid.cg_solve(h, _Field(), _Field())
    with pytest.raises(ValueError, match="multigrid.cg_solve_mixed: .* would not be a symmetric preconditioner"):
        inner = _hierarchy([(8, 16), (4, 8)], [dict(prolong="linear", faces="dirichlet"), {}])
        inner.dtype = _capi.F32
        multigrid.cg_solve_mixed(h.levels[0], inner, _Field(), _Field())


# ---------------------------------------------------------------- what the GPU tests and DESIGN 3.22 rely on: convergence
# r . r per cycle over 8 cycles of V(2, 2), damped Jacobi with omega = 0.8, 8 coarse sweeps, f64, mgcc_cases' flux-form levels on
# the plan rule's hierarchy down to extent 2, every pair Linear with the rules matched to the faces, b hashed (made compatible
# when every face is Neumann).  "mixed": Dirichlet on the low face of dimension 0 and on the high face of the last dimension,
# Neumann elsewhere.  Observed factors rr_(k-1) / rr_k, k = 1 .. 8:
#   32 x 32      Dirichlet  317, 54.0, 45.9, 42.0, 39.5, 37.9, 36.7, 35.8     Neumann  302, 59.6, 49.7, 45.2, 42.5, 40.7, 39.5, 38.6
#                mixed      315, 57.0, 47.7, 43.4, 40.8, 39.1, 37.9, 37.0
#   8 x 16 x 32  Dirichlet  329, 27.4, 20.3, 18.5, 17.5, 16.7, 16.2, 15.7     Neumann  234, 28.0, 21.2, 18.5, 16.7, 15.0, 13.1, 11.1
#                mixed      270, 28.0, 21.1, 18.8, 17.5, 16.6, 16.0, 15.5
# (the constant prolongation on the same problems: 10.1 .. 13 / 55.6 .. 112 / 8.3 .. 11.6 and 3.9 .. 12.4 / 5.9 .. 10.8 /
# 3.1 .. 8.5 over cycles 3 .. 8; the rules complemented: 9.2 .. 30 / 1.6 .. 3.0 / 1.8 .. 2.9 and 3.9 .. 30 / 1.7 .. 2.8 /
# 2.5 .. 5.0 over cycles 2 .. 8.)  The bar of each row is half its smallest factor over cycles 2 .. 8, DESIGN 3.20's rule.
def _mixed(rank):
    faces = [("neumann", "neumann")] * rank
    faces[0] = ("dirichlet", "neumann")
    faces[-1] = ("neumann", "dirichlet") if rank > 1 else ("dirichlet", "dirichlet")
    return faces


SMALLEST = {((32, 32), "dirichlet"): 35.8, ((32, 32), "neumann"): 38.6, ((32, 32), "mixed"): 37.0,
            ((8, 16, 32), "dirichlet"): 15.7, ((8, 16, 32), "neumann"): 11.1, ((8, 16, 32), "mixed"): 15.5}


def _sequence(omega, faces, linear, cycles=8):
    faces = _mixed(len(omega)) if faces == "mixed" else faces
    steps = cc.plan(omega)
    if linear:
        steps = cl.linear_steps(steps, rst.rim_of(faces, len(omega)))
    levels, _, _ = cl.flux_levels(steps, 0.8, np.float64, faces)
    assert levels[-1].m == (2,) * len(omega)
    x0, b = cl.problem(levels, faces)
    return rst.rr_sequence(levels, x0, b, cycles)


@pytest.mark.parametrize("omega,faces", list(SMALLEST), ids=[f"{len(o)}d-{f}" for o, f in SMALLEST])
def test_the_restatement_converges_with_matched_rules(omega, faces):
    seq = _sequence(omega, faces, linear=True)
    factors = [seq[k - 1] / seq[k] for k in range(1, 9)]
    print(f"{omega} {faces}: " + ", ".join(f"{f:.3g}" for f in factors))
    assert min(factors[1:]) >= 3.0, factors                    # each of cycles 2 .. 8
    assert min(factors[1:]) >= 0.5 * SMALLEST[(omega, faces)], factors


def test_linear_beats_constant_on_the_32_cubed_dirichlet_problem():
    """rr_8 / rr_0: the restatement gives 8.9e-12 with linear, 2.0e-7 with constant prolongation"""
    linear, constant = _sequence((32, 32, 32), "dirichlet", True), _sequence((32, 32, 32), "dirichlet", False)
    print(f"rr8 / rr0: linear {linear[8] / linear[0]:.3g}, constant {constant[8] / constant[0]:.3g}")
    assert linear[0] == constant[0]
    assert linear[8] / linear[0] <= 1e-3 * (constant[8] / constant[0])
