"""Multigrid on cell-centred grids without a GPU: the exported query neptune_hip_mg_halved_axes, inference and
refusals on host pointers (the argument checks run before the device is touched), the restatement's transfers as dense
matrices, the Python layer (coarsen_bounds / coarsening_plan with centring="cell", Hierarchy.halved, the error texts), and
the convergence and symmetry preconditions the GPU tests rely on -- conditions on the restatement (tests/mg_restatement.py), not
on the code under test."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_restatement as rst
import mgcc_cases as cc
from mg_restatement import Halved
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    return _capi.load()


def _geom(omega, lo=None):
    """a geometry whose Omega has extents `omega` at lower corner `lo` (default 1) in a box with a rim of one cell above"""
    lo = [1] * len(omega) if lo is None else list(lo)
    box = ([0] * len(omega), [l + m + 1 for l, m in zip(lo, omega)])
    return make_geom(box, (lo, [l + m for l, m in zip(lo, omega)]))


def _masks(lib, fine, coarse):
    """-> ((rc, mask) of neptune_hip_mg_coarsened_axes, (rc, mask) of neptune_hip_mg_halved_axes)"""
    out = []
    for fn in (lib.neptune_hip_mg_coarsened_axes, lib.neptune_hip_mg_halved_axes):
        mask = C.c_int(-7)
        rc = fn(C.byref(fine) if fine is not None else None, C.byref(coarse) if coarse is not None else None, C.byref(mask))
        out.append((rc, mask.value))
    return tuple(out)


# ---------------------------------------------------------------- the query
def test_query_is_exported_with_the_headers_signature(lib):
    name = "neptune_hip_mg_halved_axes"
    header = " ".join(_capi.HEADER_PATH.read_text().split())
    assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert ("int neptune_hip_mg_halved_axes(const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse, "
            "int *mask_out);") in header
    restype, argtypes = _capi.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == 3 and argtypes[2] is C.POINTER(C.c_int)
    assert "HALVED" in header and "m_l[d] = 2 m_(l+1)[d]:" in header


def test_halved_pairs_are_inferred_with_the_right_masks(lib):
    ok = lambda mask: ((_capi.OK, mask), (_capi.OK, mask))
    fine = _geom((6, 14, 262), (1, 2, 3))
    assert _masks(lib, fine, _geom((3, 7, 131))) == ok(0b111)
    assert _masks(lib, fine, _geom((6, 7, 131))) == ok(0b110)                  # bit d = dimension d: 1 and 2 halved, 0 kept
    assert _masks(lib, fine, _geom((6, 14, 131), (2, 1, 1))) == ok(0b100)
    assert _masks(lib, fine, _geom((3, 14, 262))) == ok(0b001)
    assert _masks(lib, fine, _geom((3, 14, 131))) == ok(0b101)
    assert _masks(lib, _geom((14, 524)), _geom((7, 262))) == ok(0b11)          # rank 2
    assert _masks(lib, _geom((14, 524)), _geom((14, 262))) == ok(0b10)
    assert _masks(lib, _geom((524,)), _geom((262,))) == ok(0b1)
    assert _masks(lib, _geom((2, 6, 130)), _geom((1, 3, 65))) == ok(0b111)     # a coarse grid one cell thick
    assert _masks(lib, _geom((2, 2)), _geom((1, 1))) == ok(0b11)
    # a vertex-centred pair: the union is the coarsened dimensions, none is halved
    assert _masks(lib, _geom((7, 15, 263)), _geom((3, 7, 131))) == ((_capi.OK, 0b111), (_capi.OK, 0))
    assert _masks(lib, _geom((7, 15, 263)), _geom((7, 7, 131))) == ((_capi.OK, 0b110), (_capi.OK, 0))


def test_query_refusals(lib):
    E = ((_capi.EINVAL, -7), (_capi.EINVAL, -7))                               # *mask_out untouched
    assert _masks(lib, _geom((6, 15, 262)), _geom((3, 7, 131))) == E           # mixed: 0 and 2 halved, 1 coarsened
    assert _masks(lib, _geom((15, 262)), _geom((7, 131))) == E
    assert _masks(lib, _geom((6, 15, 262)), _geom((6, 7, 131))) == E           # ... also beside a kept dimension
    fine = _geom((6, 14, 262))
    assert _masks(lib, fine, fine) == E                                        # all kept
    for coarse in ((3, 7, 130), (3, 8, 131), (4, 7, 131), (12, 28, 524)):      # a dimension in no state; the wrong way round
        assert _masks(lib, fine, _geom(coarse)) == E, coarse
    assert _masks(lib, fine, _geom((7, 131))) == E                             # ranks differ
    assert _masks(lib, None, fine) == E and _masks(lib, fine, None) == E
    assert lib.neptune_hip_mg_halved_axes(C.byref(fine), C.byref(_geom((3, 7, 131))), None) == _capi.EINVAL
    empty = make_geom(([0] * 3, [8, 16, 264]), ([1, 1, 1], [1, 15, 263]))
    assert _masks(lib, empty, _geom((3, 7, 131))) == E


def test_transfer_entries_refuse_bad_pairs_on_host_pointers(lib):
    """nothing may be launched: the pointers are host memory"""
    fields = [np.zeros((8, 17, 34)) for _ in range(4)]
    bf, qf, bc, xc = (a.ctypes.data for a in fields)
    E = _capi.EINVAL
    for fine, coarse in (((6, 15, 30), (3, 7, 15)),        # mixed
                         ((6, 14, 30), (6, 14, 30)),       # all kept
                         ((6, 14, 30), (3, 7, 14))):       # dimension 2 in no state
        gf, gc = _geom(fine), _geom(coarse)
        assert lib.neptune_hip_mg_restrict(_capi.F64, C.byref(gf), C.byref(gc), bf, qf, 4.0, bc, xc, None) == E, (fine, coarse)
        assert lib.neptune_hip_mg_prolong_add(_capi.F64, C.byref(gf), C.byref(gc), xc, bf, None) == E, (fine, coarse)
    # a good halved pair is refused for its other faults
    gf, gc = _geom((6, 14, 30)), _geom((3, 7, 15))
    assert lib.neptune_hip_mg_restrict(_capi.F64, C.byref(gf), C.byref(gc), bf, qf, float("nan"), bc, xc, None) == E
    assert lib.neptune_hip_mg_restrict(_capi.F64, C.byref(gf), C.byref(gc), bf, qf, 4.0, bc, bc, None) == E
    assert lib.neptune_hip_mg_prolong_add(_capi.F64, C.byref(gf), C.byref(gc), bf, bf, None) == E


def test_solve_refuses_a_mixed_pair_on_host_pointers(lib):
    def solve(omegas):
        arrays = [[np.zeros(tuple(m + 2 for m in om)) for _ in range(4)] for om in omegas]
        levels = (_capi.MgLevel * len(omegas))()
        for l, om in enumerate(omegas):
            L = levels[l]
            L.fn, L.body, L.g = None, _capi.BODY_LAP3D7_F64, _geom(om)
            L.x, L.b, L.q, L.minv = (a.ctypes.data for a in arrays[l])
            L.rscale = 4.0
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mg_solve(levels, len(omegas), _capi.F64, 2, 2, 8, 4, 1, 0.0, None, None, None, C.byref(done),
                                      C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc
    assert solve([(8, 14, 30), (4, 7, 15), (2, 3, 7)]) == _capi.EINVAL         # the second pair: 4 -> 2 halved, 7 -> 3, 15 -> 7 coarsened
    assert solve([(8, 15, 30), (4, 7, 15)]) == _capi.EINVAL
    assert solve([(8, 16, 30), (8, 16, 30)]) == _capi.EINVAL


# ---------------------------------------------------------------- the transfers as dense matrices
def _line_R(n, axes=Halved((0,))):
    where = (slice(0, n),)
    return cc.dense(lambda e: rst.restrict(e, np.zeros(n), where, 1.0, np.zeros(n // 2), np.zeros(n // 2), (slice(0, n // 2),), Halved(axes))[0],
                    n, n // 2)


def _line_P(n, axes=Halved((0,))):
    return cc.dense(lambda e: rst.prolong_add(e, (slice(0, n // 2),), np.zeros(n), (slice(0, n),), Halved(axes)), n // 2, n)


def test_dense_matrices_on_an_8_cell_line():
    R, P = _line_R(8), _line_P(8)
    want = np.zeros((4, 8))
    for j in range(4):
        want[j, 2 * j] = want[j, 2 * j + 1] = 0.5
    assert np.array_equal(R, want)                             # every row (1/2, 1/2), the boundary cells included
    assert np.array_equal(P, 2.0 * R.T)
    assert np.array_equal(P @ np.ones(4), np.ones(8))          # constants are reproduced on every cell
    assert np.array_equal(R @ np.ones(8), np.ones(4))


def test_tensor_product_against_einsum():
    """rank 3, dimensions 0 and 2 halved, 1 kept, on Omega inside a box with unequal rims: the restatement's transfers are
    the tensor products of the line matrices, P = 2^k R^T with k = 2"""
    fm, cm = (4, 3, 8), (2, 3, 4)
    fshape, cshape = (6, 6, 11), (5, 4, 6)
    fw = tuple(slice(l, l + m) for l, m in zip((1, 2, 3), fm))
    cw = tuple(slice(l, l + m) for l, m in zip((2, 1, 1), cm))
    axes = Halved((0, 2))
    d = helpers.hash_field(fshape, np.float64, seed=3)
    got_b, got_x = rst.restrict(d, np.zeros(fshape), fw, 1.0, np.full(cshape, 7.0), np.full(cshape, 7.0), cw, Halved(axes))
    R0, R2 = _line_R(4), _line_R(8)
    want = np.einsum("ai,ck,ijk->ajc", R0, R2, d[fw])
    assert np.allclose(got_b[cw], want, rtol=4e-16, atol=0) and (got_x[cw] == 0).all()
    outside = np.ones(cshape, bool)
    outside[cw] = False
    assert (got_b[outside] == 7.0).all() and (got_x[outside] == 7.0).all()
    e = helpers.hash_field(cshape, np.float64, seed=4)
    got = rst.prolong_add(e, cw, np.zeros(fshape), fw, Halved(axes))
    P0, P2 = _line_P(4), _line_P(8)
    assert np.array_equal(got[fw], np.einsum("ia,kc,ajc->ijk", P0, P2, e[cw]))
    # P = 2^k R^T as matrices on Omega
    nf, nc = int(np.prod(fm)), int(np.prod(cm))
    R = cc.dense(lambda v: rst.restrict(v.reshape(fm), np.zeros(fm), tuple(slice(0, m) for m in fm), 1.0, np.zeros(cm), np.zeros(cm),
                                            tuple(slice(0, m) for m in cm), Halved(axes))[0].reshape(-1), nf, nc)
    P = cc.dense(lambda v: rst.prolong_add(v.reshape(cm), tuple(slice(0, m) for m in cm), np.zeros(fm),
                                               tuple(slice(0, m) for m in fm), Halved(axes)).reshape(-1), nc, nf)
    assert np.array_equal(P, 4.0 * R.T)
    assert np.array_equal(P @ np.ones(nc), np.ones(nf))


def test_the_dispatch_of_the_restatement():
    """a Halved tuple goes to the cell-centred transfers, a plain one to mgsemi_cases': one hierarchy, two grid kinds"""
    d = helpers.hash_field((14,), np.float64, seed=5)
    w14, w7, w3 = (slice(0, 14),), (slice(0, 7),), (slice(0, 3),)
    b7, _ = rst.restrict(d, np.zeros(14), w14, 1.0, np.zeros(7), np.zeros(7), w7, Halved((0,)))
    assert np.array_equal(b7, 0.5 * (d[0::2] + d[1::2]))
    b3, _ = rst.restrict(b7, np.zeros(7), w7, 1.0, np.zeros(3), np.zeros(3), w3, (0,))
    assert np.allclose(b3, 0.25 * b7[0:5:2] + 0.5 * b7[1:6:2] + 0.25 * b7[2:7:2], rtol=1e-15)
    assert np.array_equal(rst.prolong_add(b3, w3, np.zeros(7), w7, (0,))[1::2], b3)
    assert np.array_equal(rst.prolong_add(b7, w7, np.zeros(14), w14, Halved((0,))), np.repeat(b7, 2))


# ---------------------------------------------------------------- the Python layer
def test_coarsen_bounds_with_cell_centring():
    from neptune_hip import multigrid
    b = ([1, 2, 3], [7, 16, 265])                              # 6 x 14 x 262
    assert multigrid.coarsen_bounds(b, centring="cell") == [3, 7, 131]
    assert multigrid.coarsen_bounds(b, axes=(1, 2), centring="cell") == [6, 7, 131]
    assert multigrid.coarsen_bounds(b, axes=[0], centring="cell") == [3, 14, 262]
    assert multigrid.coarsen_bounds(([0, 0], [2, 2]), centring="cell") == [1, 1]
    assert multigrid.coarsen_bounds(([0], [7]), centring="vertex") == [3] == multigrid.coarsen_bounds(([0], [7]))
    with pytest.raises(ValueError, match="interior extent 7 of dimension 1 is not an even number >= 2"):
        multigrid.coarsen_bounds(([0, 0], [6, 7]), centring="cell")
    multigrid.coarsen_bounds(([0, 0], [6, 7]), axes=(0,), centring="cell")         # a kept extent may be anything
    with pytest.raises(ValueError, match="interior extent 1 of dimension 0"):
        multigrid.coarsen_bounds(([0], [1]), centring="cell")
    with pytest.raises(ValueError, match="interior extent 6 of dimension 0 is not an odd number >= 3"):
        multigrid.coarsen_bounds(([0], [6]))                                          # the default stays as it is
    with pytest.raises(ValueError, match='centring is "vertex" or "cell"'):
        multigrid.coarsen_bounds(b, centring="face")
    with pytest.raises(ValueError, match="axes is empty"):
        multigrid.coarsen_bounds(b, axes=(), centring="cell")


def test_coarsening_plan_with_cell_centring_ends_at_extent_2():
    from neptune_hip import multigrid
    plan = multigrid.coarsening_plan((8, 16, 32), (1.0, 1.0, 1.0), centring="cell")
    assert [p[0] for p in plan] == [(8, 16, 32), (4, 8, 16), (2, 4, 8), (2, 2, 4), (2, 2, 2)]
    assert [p[2] for p in plan] == [(0, 1, 2), (0, 1, 2), (1, 2), (2,), ()]
    assert [p[1] for p in plan] == [(1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (4.0, 1.0, 1.0), (16.0, 4.0, 1.0)]
    assert plan == [(m, w, tuple(a)) for m, w, a in cc.plan((8, 16, 32))]          # the restated rule
    # anisotropy: the weak dimension waits, as under vertex centring
    plan = multigrid.coarsening_plan((64, 64), (0.03, 1.0), centring="cell")
    assert plan == [(m, w, tuple(a)) for m, w, a in cc.plan((64, 64), (0.03, 1.0))]
    assert [p[0] for p in plan[:4]] == [(64, 64), (64, 32), (64, 16), (64, 8)] and plan[-1][0] == (2, 2)
    assert multigrid.coarsening_plan((6, 12), (1.0, 1.0), centring="cell")[-1][0] == (3, 3)     # an odd extent ends it too
    assert multigrid.coarsening_plan((256,) * 3, (1.0,) * 3, centring="cell")[-1][0] == (2, 2, 2)
    assert multigrid.coarsening_plan((7, 15), (1.0, 1.0)) == multigrid.coarsening_plan((7, 15), (1.0, 1.0), centring="vertex")
    with pytest.raises(ValueError, match='centring is "vertex" or "cell"'):
        multigrid.coarsening_plan((8, 8), (1.0, 1.0), centring="node")


class _Like:
    """what Level and Hierarchy read of a field before anything is allocated"""

    def __init__(self, shape):
        self.shape, self.rank, self.dtype = tuple(shape), len(shape), _capi.F64
        self.lb, self.box = [0] * len(shape), ([0] * len(shape), list(shape))


@pytest.fixture()
def no_device_fields(monkeypatch):
    """Hierarchy allocates its work fields with DeviceField.empty_like: not here"""
    from neptune_hip import multigrid
    monkeypatch.setattr(multigrid.DeviceField, "empty_like", staticmethod(lambda like: None))


def _hierarchy(omegas):
    from neptune_hip import multigrid
    return multigrid.Hierarchy([multigrid.Level(None, _Like([m + 2 for m in om]), ([1] * len(om), [m + 1 for m in om]))
                                for om in omegas])


def test_hierarchy_records_halved_pairs_and_names_a_mixed_one(no_device_fields):
    h = _hierarchy([(8, 16, 264), (4, 8, 132), (2, 8, 66)])
    assert h.halved == [(0, 1, 2), (0, 2)] and h.coarsened == h.halved
    h = _hierarchy([(14,), (7,), (3,)])                        # one hierarchy, two grid kinds
    assert h.halved == [(0,), ()] and h.coarsened == [(0,), (0,)]
    h = _hierarchy([(7, 15), (7, 7)])
    assert h.halved == [()] and h.coarsened == [(1,)]
    with pytest.raises(ValueError) as err:
        _hierarchy([(8, 14, 30), (4, 7, 15), (2, 3, 7)])
    text = str(err.value)
    assert "level 2" in text and "level 1" in text and "coarsened" in text and "halved" in text
    assert "[1, 2]" in text and "[0]" in text
    with pytest.raises(ValueError, match=r"level 1, dimension 1: interior extent 6 does not nest in level 0's 15 "
                                         r"\(m_fine = 2 m_coarse \+ 1, or m_fine = m_coarse for a kept dimension\)"):
        _hierarchy([(8, 15), (4, 6)])
    with pytest.raises(ValueError, match="level 1 coarsens no dimension of level 0"):
        _hierarchy([(8, 16), (8, 16)])


# ---------------------------------------------------------------- what the GPU tests rely on: the restatement converges
# r . r per cycle over 6 cycles of V(2, 2), damped Jacobi with omega = 0.8, 8 coarse sweeps, f64, hierarchies from the plan
# rule down to extent 2, b hashed (made compatible for Neumann faces).  Observed factors rr_k / rr_(k+1), k = 0 .. 5:
#   32 x 32      Dirichlet faces  110, 42.1, 13.0, 11.5, 10.6, 10.4      Neumann faces  94.4, 112, 56.3, 66.0, 56.8, 60.8
#   8 x 16 x 32  Dirichlet faces  148, 34.5, 5.73, 12.4, 3.90, 6.79      Neumann faces  72.4, 32.8, 6.38, 10.8, 5.93, 6.92
# The bar is half the smallest factor of each row.
CONVERGENCE = {((32, 32), "dirichlet"): 10.4, ((32, 32), "neumann"): 56.3,
               ((8, 16, 32), "dirichlet"): 3.90, ((8, 16, 32), "neumann"): 5.93}


@pytest.mark.parametrize("omega,faces", list(CONVERGENCE), ids=[f"{len(o)}d-{f}" for o, f in CONVERGENCE])
def test_the_restatement_converges(omega, faces):
    levels, _, _ = cc.flux_levels(cc.plan(omega), 0.8, np.float64, faces)
    assert levels[-1].m == (2,) * len(omega)
    L0 = levels[0]
    x0, b = mgc.problem_fields(L0.shape, L0.where, np.float64)
    if faces == "neumann":
        b = cc.compatible(b, L0.where)
    seq = rst.rr_sequence(levels, x0, b, 6)
    factors = [seq[k] / seq[k + 1] for k in range(6)]
    print(f"{omega} {faces}: " + ", ".join(f"{f:.3g}" for f in factors))
    smallest = CONVERGENCE[(omega, faces)]
    assert smallest >= 3.0
    assert min(factors) >= 0.5 * smallest, factors


@pytest.mark.parametrize("faces", ["dirichlet", "neumann"])
def test_the_restated_cycle_is_a_symmetric_positive_preconditioner(faces):
    """z = M(r), one V(2, 2) cycle from z = 0: u . M(v) = v . M(u) to rounding and u . M(u) > 0 on random vectors (mean-free
    ones for Neumann faces, where constants are the operator's null space)"""
    levels, _, _ = cc.flux_levels(cc.plan((8, 16)), 0.8, np.float64, faces)
    L0 = levels[0]
    rst.start(levels)
    rng = np.random.default_rng(7)

    def vector():
        v = np.zeros(L0.shape)
        v[L0.where] = rng.standard_normal(L0.m)
        return cc.compatible(v, L0.where) if faces == "neumann" else v
    M = lambda r: rst.precondition(levels, r).copy()
    for _ in range(4):
        u, v = vector(), vector()
        Mu, Mv = M(u), M(v)
        uMv, vMu = float(np.sum(u * Mv)), float(np.sum(v * Mu))
        scale = float(np.sqrt(np.sum(u * u) * np.sum(Mv * Mv)))
        assert abs(uMv - vMu) <= 1e-12 * scale, (uMv, vMu)
        assert float(np.sum(u * Mu)) > 0 and float(np.sum(v * Mv)) > 0
