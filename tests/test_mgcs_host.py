"""The transposed linear restriction on cell-centred pairs without a GPU: the four new exports against the
header, every refusal on host pointers (the argument checks run before the device is touched), the restatement's restriction
as dense matrices against the transpose of mgcl_cases' prolongation, the symmetry of the restated cycle, the Python layer's
errors, and the iteration table DESIGN 3.23 records -- conditions on the restatement (tests/mg_restatement.py), not on the code
under test.  On the parent commit the library lacks the exports, so the fixture fails and with it every test that takes it."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_restatement as rst
import mgcc_cases as cc
import mgcl_cases as cl
import mgcs_cases as cs
from mg_restatement import EVEN, Halved, ODD, Transfers
from neptune_hip import _capi
from neptune_hip.geometry import make_geom

NEW = ("neptune_hip_mg_restrict_linear", "neptune_hip_mg_solve_transfer", "neptune_hip_mgcg_solve_transfer",
       "neptune_hip_mgcg_solve_mixed_transfer")
LIN, CONST, AVG = 1, 0, 0
RULE_PAIRS = [(EVEN, EVEN), (ODD, ODD), (EVEN, ODD), (ODD, EVEN)]


@pytest.fixture(scope="module")
def lib(built_libs):
    lib = _capi.load()
    assert all(hasattr(lib, name) for name in NEW)
    return lib


def _geom(omega, lo=None):
    lo = [1] * len(omega) if lo is None else list(lo)
    box = ([0] * len(omega), [l + m + 1 for l, m in zip(lo, omega)])
    return make_geom(box, (lo, [l + m for l, m in zip(lo, omega)]))


def _transfer(prolong, restrict, lo=(0, 0, 0), hi=(0, 0, 0)):
    t = _capi.MgTransfer()
    t.prolong, t.restrict_kind = prolong, restrict
    for d in range(3):
        t.rim_lo[d], t.rim_hi[d] = lo[d], hi[d]
    return t


# ---------------------------------------------------------------- exports and prototypes
def test_exports_and_prototypes_match_the_header(lib):
    header = " ".join(_capi.HEADER_PATH.read_text().split())
    for text in ("#define NEPTUNE_HIP_MG_RESTRICT_AVERAGE 0", "#define NEPTUNE_HIP_MG_RESTRICT_LINEAR 1",
                 "typedef struct { int32_t prolong, restrict_kind; int32_t rim_lo[3], rim_hi[3]; } neptune_hip_mg_transfer_t;",
                 "int neptune_hip_mg_restrict_linear(int dtype, const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t "
                 "*g_coarse, const neptune_hip_mg_transfer_t *t, const void *b_fine, const void *q_fine, double rscale, void *b_coarse, "
                 "void *x_coarse, void *stream);",
                 "int neptune_hip_mg_solve_transfer(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, const "
                 "neptune_hip_mg_transfer_t *transfer, int n_levels, int dtype, int pre, int post, int coarse_sweeps, int64_t max_cycles, "
                 "int64_t check_every, double tol2, double *rr_checks, void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t "
                 "*cycles_done, double *rr0, double *rr_last);",
                 "int neptune_hip_mgcg_solve_transfer(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, const "
                 "neptune_hip_mg_transfer_t *transfer, int n_levels, int dtype, neptune_hip_apply_dot_fn fn_dot, int sweeps, int "
                 "coarse_sweeps, void *const work[3], int64_t max_iters, int64_t check_every, double tol2, void *trace, void *stream, "
                 "const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done, double *rr0, double *rr_last);",
                 "int neptune_hip_mgcg_solve_mixed_transfer(const neptune_hip_mg_level_t *outer, int dtype_outer, neptune_hip_apply_dot_fn "
                 "fn_dot, const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, const neptune_hip_mg_transfer_t "
                 "*transfer, int n_levels, int dtype_inner, int sweeps, int coarse_sweeps, void *const work[2], int64_t max_iters, int64_t "
                 "check_every, double tol2, void *trace, void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done, double "
                 "*rr0, double *rr_last);",
                 "s_m = 0.25 * a_m; p_0 = 0.75 * a[2 j]; p_1 = 0.75 * a[2 j + 1]; s_p = 0.25 * a_p",
                 "u = s_m + p_0; v = p_1 + s_p; w = u + v; t = 0.5 * w"):
        assert text in header, text
    assert (_capi.MG_RESTRICT_AVERAGE, _capi.MG_RESTRICT_LINEAR) == (0, 1)
    assert C.sizeof(_capi.MgTransfer) == 32
    assert [f[0] for f in _capi.MgTransfer._fields_] == ["prolong", "restrict_kind", "rim_lo", "rim_hi"]
    assert (_capi.MgTransfer.prolong.offset, _capi.MgTransfer.restrict_kind.offset, _capi.MgTransfer.rim_lo.offset,
            _capi.MgTransfer.rim_hi.offset) == (0, 4, 8, 20)
    tp = C.POINTER(_capi.MgTransfer)
    restype, args = _capi.SIGNATURES["neptune_hip_mg_restrict_linear"]
    plain = _capi.SIGNATURES["neptune_hip_mg_restrict"][1]
    assert restype is C.c_int and args[:3] == plain[:3] and args[3] is tp and args[4:] == plain[3:]
    for new, old, at in (("neptune_hip_mg_solve_transfer", "neptune_hip_mg_solve_lines", 2),
                         ("neptune_hip_mgcg_solve_transfer", "neptune_hip_mgcg_solve_lines", 2),
                         ("neptune_hip_mgcg_solve_mixed_transfer", "neptune_hip_mgcg_solve_mixed", 5)):
        restype, args = _capi.SIGNATURES[new]
        was = _capi.SIGNATURES[old][1]
        assert restype is C.c_int and args[:at] == was[:at] and args[at] is tp and args[at + 1:] == was[at:], new


# ---------------------------------------------------------------- refusals on host pointers: nothing may be launched
def test_the_kernel_entry_refuses_on_host_pointers(lib):
    bf, qf = np.full((8, 16, 32), 3.0), np.full((8, 16, 32), 2.0)
    bc, xc = np.full((5, 9, 17), 5.0), np.full((5, 9, 17), 6.0)
    gf, gc = _geom((6, 14, 30)), _geom((3, 7, 15))
    E, f64 = _capi.EINVAL, _capi.F64

    def call(t, g_fine=gf, g_coarse=gc, b_fine=bf, q_fine=qf, b_coarse=bc, x_coarse=xc, dtype=f64, rscale=4.0):
        return lib.neptune_hip_mg_restrict_linear(dtype, C.byref(g_fine), C.byref(g_coarse), C.byref(t) if t is not None else None,
                                                  b_fine.ctypes.data, q_fine.ctypes.data, rscale, b_coarse.ctypes.data,
                                                  x_coarse.ctypes.data, None)
    assert call(None) == E
    for bad in (2, -1):                                                                # a kind outside {0, 1}, either transfer
        assert call(_transfer(CONST, bad)) == E and call(_transfer(bad, LIN)) == E and call(_transfer(bad, AVG)) == E
    for prolong, restrict in ((CONST, LIN), (LIN, LIN), (LIN, AVG)):                   # a rule outside {0, 1} when either is LINEAR
        for d in range(3):
            for bad in (2, -1):
                lo, hi = [0, 1, 0], [1, 0, 1]
                lo[d] = bad
                assert call(_transfer(prolong, restrict, lo=lo, hi=[1, 0, 1])) == E, (d, bad)
                hi[d] = bad
                assert call(_transfer(prolong, restrict, lo=[0, 1, 0], hi=hi)) == E, (d, bad)
    # ... also on a dimension the pair keeps (dimension 0 here): it is a dimension < rank
    assert call(_transfer(CONST, LIN, lo=(7, 0, 0)), g_coarse=_geom((6, 7, 15))) == E
    # LINEAR on a pair with no halved dimension: a vertex-centred one
    assert call(_transfer(CONST, LIN), g_fine=_geom((7, 15, 31))) == E
    assert call(_transfer(LIN, AVG), g_fine=_geom((7, 15, 31))) == E
    # what neptune_hip_mg_restrict refuses, for either kind
    for t in (_transfer(LIN, LIN), _transfer(CONST, LIN), _transfer(CONST, AVG)):
        assert call(t, g_fine=_geom((6, 15, 30))) == E                                 # halved and coarsened in one pair
        assert call(t, g_fine=gc, g_coarse=gc) == E                                    # all kept
        assert call(t, g_coarse=_geom((3, 7, 14))) == E                                # dimension 2 in no state
        assert call(t, g_coarse=_geom((7, 15))) == E                                   # ranks differ
        assert call(t, b_coarse=bf) == E and call(t, x_coarse=qf) == E                 # a written field overlaps a read one
        assert call(t, x_coarse=bc) == E                                               # the two written fields overlap
        assert call(t, dtype=7) == E
        assert call(t, rscale=float("inf")) == E and call(t, rscale=float("nan")) == E
    assert (bf == 3.0).all() and (qf == 2.0).all() and (bc == 5.0).all() and (xc == 6.0).all()


def _solve_args(omegas, body=_capi.BODY_LAP3D7_F64, dtype=np.float64):
    arrays = [[np.full(tuple(m + 2 for m in om), 1.5, dtype) for _ in range(4)] for om in omegas]
    levels = (_capi.MgLevel * len(omegas))()
    for l, om in enumerate(omegas):
        L = levels[l]
        L.fn, L.body, L.g = None, body, _geom(om)
        L.x, L.b, L.q, L.minv = (a.ctypes.data for a in arrays[l])
        L.rscale = 4.0
    return levels, arrays


GOOD = [(8, 16, 32), (4, 8, 16), (2, 4, 8)]
OK = [_transfer(LIN, LIN, (1, 1, 1), (1, 1, 1)), _transfer(LIN, LIN)]


def _array(transfer):
    return None if transfer is None else (_capi.MgTransfer * len(transfer))(*transfer)


def _plain(lib):
    def solve(omegas, transfer, n_levels=None, max_cycles=4, check_every=1, pre=2, lines=None, body=_capi.BODY_LAP3D7_F64):
        levels, arrays = _solve_args(omegas, body)
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mg_solve_transfer(levels, lines, _array(transfer), len(omegas) if n_levels is None else n_levels, _capi.F64,
                                               pre, 2, 8, max_cycles, check_every, 0.0, None, None, None, C.byref(done), C.byref(rr0),
                                               C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        assert all((a == 1.5).all() for level in arrays for a in level), "a refusal leaves every field's bits unchanged"
        return rc
    return solve


def _cg(lib):
    def solve(omegas, transfer, n_levels=None, max_iters=4, check_every=1, sweeps=2, lines=None, body=_capi.BODY_LAP3D7_F64, work=True):
        levels, arrays = _solve_args(omegas, body)
        wk = [np.full(arrays[0][0].shape, 2.5) for _ in range(3)]
        warr = (C.c_void_p * 3)(*[a.ctypes.data for a in wk]) if work else None
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mgcg_solve_transfer(levels, lines, _array(transfer), len(omegas) if n_levels is None else n_levels, _capi.F64,
                                                 None, sweeps, 8, warr, max_iters, check_every, 0.0, None, None, None, C.byref(done),
                                                 C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        assert all((a == 1.5).all() for level in arrays for a in level) and all((a == 2.5).all() for a in wk)
        return rc
    return solve


def _mixed(lib):
    def solve(omegas, transfer, n_levels=None, max_iters=4, check_every=1, sweeps=2, lines=None, dtype_outer=_capi.F64, work=True):
        levels, arrays = _solve_args(omegas, _capi.BODY_LAP3D27_F32, np.float32)
        outer, oarrays = _solve_args(omegas[:1])
        wk = [np.full(oarrays[0][0].shape, 2.5) for _ in range(2)]
        warr = (C.c_void_p * 2)(*[a.ctypes.data for a in wk]) if work else None
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mgcg_solve_mixed_transfer(outer, dtype_outer, None, levels, lines, _array(transfer),
                                                       len(omegas) if n_levels is None else n_levels, _capi.F32, sweeps, 8, warr, max_iters,
                                                       check_every, 0.0, None, None, None, C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        assert all((a == 1.5).all() for level in arrays + oarrays for a in level) and all((a == 2.5).all() for a in wk)
        return rc
    return solve


@pytest.mark.parametrize("entry", ["plain", "cg", "mixed"])
def test_the_solves_refuse_on_host_pointers(lib, entry):
    solve = {"plain": _plain, "cg": _cg, "mixed": _mixed}[entry](lib)
    E = _capi.EINVAL
    # the new refusals, on either pair
    for l in range(2):
        for bad in (_transfer(LIN, 2), _transfer(LIN, -3), _transfer(2, LIN), _transfer(LIN, LIN, lo=(0, 2, 0)),
                    _transfer(LIN, LIN, hi=(0, 0, -1)), _transfer(CONST, LIN, lo=(0, 2, 0))):
            transfer = list(OK)
            transfer[l] = bad
            assert solve(GOOD, transfer) == E, (l, bad.prolong, bad.restrict_kind)
    assert solve([(8, 16, 32), (8, 8, 16), (4, 4, 8)], [_transfer(LIN, LIN, lo=(5, 0, 0)), _transfer(LIN, LIN)]) == E   # a kept dimension
    assert solve([(7, 15, 31), (3, 7, 15)], [_transfer(CONST, LIN)]) == E              # LINEAR restriction on a vertex-centred pair
    assert solve([(7, 15, 31), (3, 7, 15)], [_transfer(LIN, LIN)]) == E
    assert solve([(14, 14, 14), (7, 7, 7), (3, 3, 3)], [_transfer(LIN, LIN), _transfer(LIN, LIN)]) == E      # ... on the second pair only
    # every refusal of the entry being extended, with the array present -- and with NULL and an all-default array, which are
    # accepted wherever the extended entry accepts and so must not add a refusal of their own
    for transfer in (OK, None, [_transfer(CONST, AVG)] * 2):
        assert solve([(8, 15, 32), (4, 7, 16)], transfer and transfer[:1]) == E        # a mixed pair
        assert solve([(8, 16, 32), (8, 16, 32)], transfer and transfer[:1]) == E       # all kept
        assert solve(GOOD, transfer, n_levels=0) == E and solve(GOOD, transfer, n_levels=17) == E
        assert solve(GOOD, transfer, check_every=0) == E
        stages = (_capi.MgLines * 3)()
        stages[1].n_stages = 4
        assert solve(GOOD, transfer, lines=stages) == E
        stages[1].n_stages = 1
        stages[1].axis[0] = 3
        assert solve(GOOD, transfer, lines=stages) == E
        if entry == "plain":
            assert solve(GOOD, transfer, max_cycles=-1) == E and solve(GOOD, transfer, pre=-1) == E
            assert solve(GOOD, transfer, body=_capi.BODY_LAP3D27_F32) == E             # a built-in body of another element type
        else:
            assert solve(GOOD, transfer, max_iters=-1) == E and solve(GOOD, transfer, sweeps=0) == E
            assert solve(GOOD, transfer, n_levels=1) == E and solve(GOOD, transfer, work=False) == E
        if entry == "cg":
            assert solve(GOOD, transfer, body=_capi.BODY_LAP3D27_F32) == E
        if entry == "mixed":
            assert solve(GOOD, transfer, dtype_outer=_capi.F32) == E
    # the asymmetric pairs: the plain solve takes them (that reaches the device: test_mgcs_solve_gpu.py), the CG entries refuse
    if entry != "plain":
        for l in range(2):
            for bad in (_transfer(LIN, AVG, (1, 1, 1), (1, 1, 1)), _transfer(CONST, LIN)):
                transfer = list(OK)
                transfer[l] = bad
                assert solve(GOOD, transfer) == E, (l, bad.prolong, bad.restrict_kind)


# ---------------------------------------------------------------- the restriction as dense matrices
def _line_R(n, rule_lo, rule_hi):
    axes = Transfers((0,), ((rule_lo, rule_hi),))
    w_f, w_c = (slice(0, n),), (slice(0, n // 2),)
    return cc.dense(lambda e: rst.restrict(e, np.zeros(n), w_f, 1.0, np.zeros(n // 2), np.zeros(n // 2), w_c, axes)[0], n, n // 2)


def _line_P(n, rule_lo, rule_hi):
    axes = rst.Linear((0,), ((rule_lo, rule_hi),))
    return cc.dense(lambda e: rst.prolong_add(e, (slice(0, n // 2),), np.zeros(n), (slice(0, n),), axes), n // 2, n)


@pytest.mark.parametrize("rule_lo,rule_hi", RULE_PAIRS)
def test_dense_matrix_on_a_16_to_8_line_is_half_the_transpose(rule_lo, rule_hi):
    R, P = _line_R(16, rule_lo, rule_hi), _line_P(16, rule_lo, rule_hi)
    assert R.shape == (8, 16)
    assert np.array_equal(R, P.T / 2.0)                        # exactly: the weights are dyadic
    want = np.zeros((8, 16))
    for j in range(1, 7):
        want[j, 2 * j - 1:2 * j + 3] = (0.125, 0.375, 0.375, 0.125)
    want[0, :3] = (0.5 if rule_lo == EVEN else 0.25, 0.375, 0.125)
    want[7, 13:] = (0.125, 0.375, 0.5 if rule_hi == EVEN else 0.25)
    assert np.array_equal(R, want)
    if (rule_lo, rule_hi) == (EVEN, EVEN):
        assert np.array_equal(R @ np.ones(16), np.ones(8))     # constants are restricted exactly on every cell


def test_a_one_cell_coarse_line_has_two_ghosts():
    for rule_lo, rule_hi in RULE_PAIRS:
        want = [0.5 if rule_lo == EVEN else 0.25, 0.5 if rule_hi == EVEN else 0.25]
        assert np.array_equal(_line_R(2, rule_lo, rule_hi), np.array(want).reshape(1, 2))
        assert np.array_equal(_line_R(2, rule_lo, rule_hi), _line_P(2, rule_lo, rule_hi).T / 2.0)


def _dyadic(rng, shape):
    return rng.integers(-64, 64, shape) / 8.0                  # every product with 3/4, 1/4, 1/2 and every sum is exact


@pytest.mark.parametrize("fm,axes,rim", [((6, 8), (0, 1), ((ODD, EVEN), (EVEN, ODD))),
                                         ((4, 6, 8), (0, 1, 2), ((ODD, EVEN), (ODD, ODD), (EVEN, ODD))),
                                         ((4, 3, 8), (0, 2), ((EVEN, ODD), (ODD, ODD), (ODD, EVEN)))],        # dimension 1 kept
                         ids=["2d", "3d", "kept-axis"])
def test_transposition_and_tensor_product_on_dyadic_data(fm, axes, rim):
    """<P e, f> == 2^k <e, R f> with ==, and R against the tensor product of the line matrices, on small-integer data; Omega
    inside boxes with unequal rims holding NaN outside the fine Omega"""
    rank, k = len(fm), len(axes)
    cm = tuple(m // 2 if d in axes else m for d, m in enumerate(fm))
    fshape, cshape = tuple(m + 3 + d for d, m in enumerate(fm)), tuple(m + 2 + d for d, m in enumerate(cm))
    fw = tuple(slice(1 + d, 1 + d + m) for d, m in enumerate(fm))
    cw = tuple(slice(2, 2 + m) for m in cm)
    rng = np.random.default_rng(13)
    marker = Transfers(axes, rim)
    f = np.full(fshape, np.nan)
    f[fw] = _dyadic(rng, fm)
    q = np.full(fshape, np.nan)
    q[fw] = 0.0
    e = np.zeros(cshape)
    e[cw] = _dyadic(rng, cm)
    b_c, x_c = rst.restrict(f, q, fw, 1.0, np.full(cshape, 7.0), np.full(cshape, 9.0), cw, marker)
    Pe = rst.prolong_add(e, cw, np.zeros(fshape), fw, marker)
    assert float(np.sum(Pe[fw] * f[fw])) == 2.0 ** k * float(np.sum(e[cw] * b_c[cw]))
    outside = np.ones(cshape, bool)
    outside[cw] = False
    assert (b_c[outside] == 7.0).all() and (x_c[outside] == 9.0).all() and (x_c[cw] == 0.0).all() and not np.signbit(x_c[cw]).any()
    mats = [_line_R(fm[d], *rim[d]) if d in axes else np.eye(fm[d]) for d in range(rank)]
    if rank == 2:
        want = np.einsum("ia,jb,ab->ij", *mats, f[fw])
    else:
        want = np.einsum("ia,jb,kc,abc->ijk", *mats, f[fw])
    assert np.array_equal(b_c[cw], want)
    # rscale enters as one exact scaling here
    b4, _ = rst.restrict(f, q, fw, 4.0, np.full(cshape, 7.0), np.full(cshape, 9.0), cw, marker)
    assert np.array_equal(b4[cw], 4.0 * want)


def test_the_ghost_is_an_exact_sign_flip_and_keeps_minus_zero():
    """a fine line of -0 under (ODD, EVEN): the low ghost is +0, so the first coarse cell is (+0 + -0) + ... = +0, while every
    other coarse cell, the high one with its EVEN ghost -0 included, adds -0 only and stays -0"""
    d = np.full(8, -0.0)
    w8, w4 = (slice(0, 8),), (slice(0, 4),)
    b, x = rst.restrict(d, np.zeros(8), w8, 1.0, np.ones(4), np.ones(4), w4, Transfers((0,), ((ODD, EVEN),)))
    assert list(np.signbit(b)) == [False, True, True, True] and (b == 0).all()
    assert (x == 0).all() and not np.signbit(x).any()
    # the corner weight in two dimensions is the product of the two end rows: the ghost of the later dimension is +- the
    # intermediate at the edge
    one = np.zeros((4, 4))
    one[0, 0] = 1.0
    w44, w22 = (slice(0, 4),) * 2, (slice(0, 2),) * 2
    corner, _ = rst.restrict(one, np.zeros((4, 4)), w44, 1.0, np.zeros((2, 2)), np.zeros((2, 2)), w22,
                            Transfers((0, 1), ((ODD, EVEN), (ODD, EVEN))))
    assert corner[0, 0] == 0.25 * 0.25 and corner[0, 1] == 0.0 and corner[1, 1] == 0.0
    one[0, 0], one[3, 3] = 0.0, 1.0
    corner, _ = rst.restrict(one, np.zeros((4, 4)), w44, 1.0, np.zeros((2, 2)), np.zeros((2, 2)), w22,
                            Transfers((0, 1), ((ODD, EVEN), (ODD, EVEN))))
    assert corner[1, 1] == 0.5 * 0.5


def test_the_dispatch_of_the_restatement():
    """a Transfers marker goes by its two choices; anything else is mgcl_cases'"""
    d = helpers.hash_field((14,), np.float64, seed=5)
    w14, w7 = (slice(0, 14),), (slice(0, 7),)
    rim = ((EVEN, ODD),)
    args = (d, np.zeros(14), w14, 1.0, np.zeros(7), np.zeros(7), w7)
    avg = 0.5 * (d[0::2] + d[1::2])
    sym = Transfers((0,), rim)
    assert sym.halved and sym == (0,) and sym.rim == rim and sym.symmetric
    assert not Transfers((0,), rim, "constant", "linear").symmetric and Transfers((0,), rim, "constant", "average").symmetric
    assert np.array_equal(rst.restrict(*args, Halved((0,)))[0], avg)
    assert np.array_equal(rst.restrict(*args, rst.Linear((0,), rim))[0], avg)
    assert np.array_equal(rst.restrict(*args, Transfers((0,), rim, "linear", "average"))[0], avg)
    got = rst.restrict(*args, sym)[0]
    assert got[2] == 0.5 * ((0.25 * d[3] + 0.75 * d[4]) + (0.75 * d[5] + 0.25 * d[6]))
    assert got[0] == 0.5 * ((0.25 * d[0] + 0.75 * d[0]) + (0.75 * d[1] + 0.25 * d[2]))
    assert got[6] == 0.5 * ((0.25 * d[11] + 0.75 * d[12]) + (0.75 * d[13] + 0.25 * -d[13]))
    assert np.array_equal(rst.restrict(*args, Transfers((0,), rim, "constant", "linear"))[0], got)
    e = got
    assert np.array_equal(rst.prolong_add(e, w7, np.zeros(14), w14, Transfers((0,), rim, "constant", "linear")), np.repeat(e, 2))
    assert np.array_equal(rst.prolong_add(e, w7, np.zeros(14), w14, sym), rst.prolong_add(e, w7, np.zeros(14), w14, rst.Linear((0,), rim)))
    assert rst.transfer_of(sym, 1) == (1, 1, [EVEN], [ODD]) and rst.transfer_of(Halved((0,)), 2) == (0, 0, [0, 0], [0, 0])
    assert rst.transfer_of(rst.Linear((0,), rim), 1) == (1, 0, [EVEN], [ODD])


# ---------------------------------------------------------------- the restated cycle is a symmetric positive preconditioner
def _mixed_faces(rank):
    faces = [("neumann", "neumann")] * rank
    faces[0] = ("dirichlet", "neumann")
    faces[-1] = ("neumann", "dirichlet") if rank > 1 else ("dirichlet", "dirichlet")
    return faces


def _faces(name, rank):
    return _mixed_faces(rank) if name == "mixed" else name


@pytest.mark.parametrize("faces", ["dirichlet", "mixed"])
def test_the_restated_cycle_is_a_symmetric_positive_preconditioner(faces):
    """z = M(r), one V(2, 2) cycle from z = 0 with the symmetric linear pair on every pair: u . M(v) = v . M(u) to rounding and
    u . M(u) > 0 on random vectors -- the check test_mgcc_host.py makes for the constant pair, with its bound; the
    linear / averaging pair of DESIGN 3.22 misses that bound by orders of magnitude"""
    f = _faces(faces, 2)
    rim = rst.rim_of(f, 2)
    rng = np.random.default_rng(7)

    def asymmetry(steps):
        levels, _, _ = cs.flux_levels(steps, 0.8, np.float64, f)
        L0 = levels[0]
        rst.start(levels)
        worst = 0.0
        for _ in range(4):
            u, v = np.zeros(L0.shape), np.zeros(L0.shape)
            u[L0.where], v[L0.where] = rng.standard_normal(L0.m), rng.standard_normal(L0.m)
            Mu, Mv = rst.precondition(levels, u).copy(), rst.precondition(levels, v).copy()
            uMv, vMu = float(np.sum(u * Mv)), float(np.sum(v * Mu))
            assert float(np.sum(u * Mu)) > 0 and float(np.sum(v * Mv)) > 0
            worst = max(worst, abs(uMv - vMu) / float(np.sqrt(np.sum(u * u) * np.sum(Mv * Mv))))
        return worst
    assert asymmetry(cs.transfer_steps(cc.plan((8, 16)), rim)) <= 1e-12
    assert asymmetry(cl.linear_steps(cc.plan((8, 16)), rim)) >= 1e-6


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
    sym = dict(prolong="linear", restrict="linear")
    h = _hierarchy([(8, 16, 32), (4, 8, 16), (2, 8, 8), (1, 4, 4)],
                   [dict(faces="dirichlet", **sym), {},
                    dict(faces=[("neumann", "dirichlet"), ("dirichlet", "dirichlet"), ("neumann", "neumann")], restrict="linear"),
                    dict(restrict="linear")])              # the last level's setting is ignored, faces missing or not
    assert h.has_linear_restrict and h.has_linear and not h.symmetric
    assert [L.restrict_linear for L in h.levels] == [True, False, True, True]
    arr = h._transfer_structs()
    assert len(arr) == 3
    assert [(t.prolong, t.restrict_kind, list(t.rim_lo), list(t.rim_hi)) for t in arr] == [
        (1, 1, [1, 1, 1], [1, 1, 1]), (0, 0, [0, 0, 0], [0, 0, 0]), (0, 1, [0, 1, 0], [1, 1, 0])]
    h2 = _hierarchy([(8, 16), (4, 8), (2, 4)], [dict(faces="neumann", **sym), {}, dict(restrict="linear")])
    assert h2.symmetric and h2.has_linear_restrict
    assert [(t.prolong, t.restrict_kind) for t in h2._transfer_structs()] == [(1, 1), (0, 0)]
    plain = _hierarchy([(8, 16), (4, 8)], [{}, dict(restrict="linear")])
    assert plain.symmetric and not plain.has_linear_restrict and not plain.has_linear
    lin = _hierarchy([(8, 16), (4, 8)], [dict(prolong="linear", faces="neumann"), {}])
    assert not lin.symmetric and not lin.has_linear_restrict and lin.has_linear


def test_hierarchy_names_the_level_of_a_bad_setting(no_device_fields):
    good = [(8, 16), (4, 8), (2, 4)]
    with pytest.raises(ValueError, match=r'level 1: restrict="linear" needs faces'):
        _hierarchy(good, [{}, dict(restrict="linear"), {}])
    with pytest.raises(ValueError, match=r'level 1: prolong="linear" needs faces'):
        _hierarchy(good, [{}, dict(prolong="linear", restrict="linear"), {}])
    with pytest.raises(ValueError, match=r"level 0: faces is .* not "):
        _hierarchy(good, [dict(restrict="linear", faces="periodic"), {}, {}])
    with pytest.raises(ValueError, match=r'level 1: restrict is "average" or "linear", not \'cubic\''):
        _hierarchy(good, [{}, dict(restrict="cubic"), {}])
    with pytest.raises(ValueError, match=r'level 1: restrict="linear" needs a cell-centred pair, but no dimension is halved towards level 2'):
        _hierarchy([(14, 14), (7, 7), (3, 3)], [dict(restrict="linear", faces="dirichlet"), dict(restrict="linear", faces="dirichlet"), {}])
    _hierarchy([(14, 14), (7, 7), (3, 3)], [dict(restrict="linear", faces="dirichlet"), {}, {}])


def test_cg_solve_accepts_the_symmetric_pair_and_refuses_the_others(no_device_fields, monkeypatch):
    from neptune_hip import multigrid
    sym = _hierarchy([(8, 16), (4, 8)], [dict(prolong="linear", restrict="linear", faces="dirichlet"), {}])

    class _Field:
        box, dtype = sym.levels[0].like.box, _capi.F64

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    # past every check of the hierarchy the call builds its C structs: that is where the stub stops it
    monkeypatch.setattr(multigrid.Hierarchy, "_structs", stop)
    with pytest.raises(Reached):
        multigrid.cg_solve(sym, _Field(), _Field(), work=[None] * 3)
    for settings in (dict(prolong="linear", faces="dirichlet"), dict(restrict="linear", faces="dirichlet")):
        h = _hierarchy([(8, 16), (4, 8)], [settings, {}])
        with pytest.raises(ValueError, match=r'would not be a symmetric preconditioner.*restrict="linear"'):
            multigrid.cg_solve(h, _Field(), _Field())
        with pytest.raises(ValueError, match="multigrid.cg_solve_mixed: .* would not be a symmetric preconditioner"):
            inner = _hierarchy([(8, 16), (4, 8)], [settings, {}])
            inner.dtype = _capi.F32
            multigrid.cg_solve_mixed(h.levels[0], inner, _Field(), _Field())


# ---------------------------------------------------------------- the iteration table of DESIGN 3.23
# cg_solve restated (mg_restatement.numpy_mgcg: the project's bit-exact cycle, numpy's own sums for the scalars), f64, mgcc_cases'
# flux-form levels on the plan rule's hierarchy down to extent 2, damped Jacobi with omega = 0.8 in two dimensions and 6 / 7
# in three, 8 coarse sweeps, x = 0, b hashed: the first iteration with r . r <= 1e-16 rr_0.  "mixed": Dirichlet on the low face
# of dimension 0 and on the high face of the last dimension, Neumann elsewhere.  The symmetric pair carries the rules matched
# to the faces on every pair.  (omega, faces, sweeps): (constant / averaging pair, symmetric linear pair)
ITERATIONS = {
    ((32, 32), "dirichlet", 1): (15, 10), ((32, 32), "dirichlet", 2): (9, 8),
    ((32, 32), "mixed", 1): (15, 10), ((32, 32), "mixed", 2): (9, 8),
    ((8, 16, 32), "dirichlet", 1): (17, 11), ((8, 16, 32), "dirichlet", 2): (10, 9),
    ((8, 16, 32), "mixed", 1): (18, 11), ((8, 16, 32), "mixed", 2): (11, 8),
    ((32, 32, 32), "dirichlet", 1): (20, 12), ((32, 32, 32), "dirichlet", 2): (11, 9),
    ((32, 32, 32), "mixed", 1): (22, 12), ((32, 32, 32), "mixed", 2): (12, 9),
}


@pytest.mark.parametrize("omega,faces,sweeps", list(ITERATIONS), ids=[f"{'x'.join(map(str, o))}-{f}-V{s}{s}" for o, f, s in ITERATIONS])
def test_the_iteration_table(omega, faces, sweeps):
    rank = len(omega)
    f = _faces(faces, rank)
    damp = 0.8 if rank == 2 else 6.0 / 7.0
    steps = cc.plan(omega)
    constant = cs.mgcg_iterations(steps, f, damp, sweeps)
    symmetric = cs.mgcg_iterations(cs.transfer_steps(steps, rst.rim_of(f, rank)), f, damp, sweeps)
    print(f"{omega} {faces} V({sweeps},{sweeps}): constant {constant}, symmetric linear {symmetric}")
    assert (constant, symmetric) == ITERATIONS[(omega, faces, sweeps)]
    assert symmetric <= constant
