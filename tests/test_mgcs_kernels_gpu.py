"""The transposed linear restriction kernel of a cell-centred pair alone (neptune_hip_mg_restrict_linear)
against the NumPy restatement of tests/mg_restatement.py: bit for bit on every cell of b_c and x_c, the untouched cells outside the
coarse Omega included.  On the parent commit the library lacks the export, so every test here fails there.

Shapes: those of test_mgcl_kernels_gpu.py -- rank 3, fine box 9 x 18 x 268, Omega 6 x 14 x 262 at (1, 2, 3) onto 3 x 7 x 131 under
each of the 7 subsets of halved axes; an even corner; a box of odd pitch 269; rank 2, 14 x 524 onto 7 x 262; rank 1; `thin`,
whose coarse Omega is 1 x 3 x 65; `long`, Omega 2 x 4 x 524 -> 1 x 2 x 262, a coarse row beyond one 256-cell chunk with m_c = 1 on
dimension 0 -- and `runs`, Omega 4 x 36 x 12 -> 2 x 18 x 6: the kernel marches runs of 8 coarse rows along axis 1 and carries the
last four fine rows in registers, so 18 coarse rows give two full runs and a short one.  f64 and f32.

Every case runs under a pattern of rules and under its complement, so every face meets EVEN and ODD.
test_the_cases_reach_every_path computes from the cases themselves that the aligned and the misaligned pair loads, the
wave-edge lanes, a chunk boundary inside a row, a run boundary inside a plane and both ghost ends on every axis are reached.

b_f and q_f hold -0 in places and NaN on every cell outside the fine Omega: a NaN in the output is a cell read that must not
be.  b_c and x_c hold sentinels that must survive outside the coarse Omega."""
import ctypes as C
import itertools

import numpy as np
import pytest

import helpers
import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import dev
from mg_restatement import EVEN, Halved, ODD, Transfers

pytestmark = pytest.mark.gpu

R3 = ((9, 18, 268), (1, 2, 3), (6, 14, 262))      # fine box, fine Omega's lower corner, fine Omega
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(range(3), n)]
# name: (fine box, fine Omega's lower corner, fine Omega, the dimensions halved, coarse Omega's lower corner)
CASES = {"r3-" + "".join(map(str, s)): R3 + (s, (1, 1, 2)) for s in SUBSETS}
CASES.update({
    "even-corner": ((9, 18, 268), (1, 2, 2), (6, 14, 262), (0, 1, 2), (2, 1, 2)),
    "odd-pitch": ((9, 18, 269), (1, 2, 3), (6, 14, 262), (0, 1, 2), (1, 2, 1)),
    "r2": ((17, 528), (1, 2), (14, 524), (0, 1), (2, 1)),
    "r2-1": ((17, 528), (1, 2), (14, 524), (1,), (1, 3)),
    "r1": ((530,), (3,), (524,), (0,), (2,)),
    "thin": ((4, 8, 133), (1, 1, 2), (2, 6, 130), (0, 1, 2), (1, 2, 1)),            # coarse Omega 1 x 3 x 65
    "long": ((4, 7, 530), (1, 2, 3), (2, 4, 524), (0, 1, 2), (1, 1, 2)),            # coarse Omega 1 x 2 x 262
    "runs": ((6, 39, 15), (1, 2, 1), (4, 36, 12), (0, 1, 2), (1, 1, 1)),            # coarse Omega 2 x 18 x 6
})
F64, F32 = np.float64, np.float32
RUN = 8                                            # kMgLinearRun: coarse rows per workgroup along axis 1
PATTERN = ((EVEN, ODD), (ODD, EVEN), (EVEN, EVEN))     # per dimension (low, high), the last `rank` entries read from the right
RUNS = [(n, d, 8) for n in CASES if n != "even-corner" for d in (F64, F32)] + \
       [(n, d, 0) for n in ("r3-012", "even-corner", "odd-pitch") for d in (F64, F32)]
IDS = lambda runs: [f"{n}-{np.dtype(d).name}" + ("-offset" if o else "") for n, d, o in runs]


def _rim(name, complemented):
    rank = len(CASES[name][0])
    rim = (PATTERN * 2)[3 - rank + (1 if name == "thin" else 0):][:rank]       # `thin` shifted: another face meets ODD first
    return rst.complement(rim) if complemented else tuple(rim)


def _coarse(name):
    fbox, flo, fm, axes, clo = CASES[name]
    return tuple(m // 2 if d in axes else m for d, m in enumerate(fm))


def test_the_cases_reach_every_path():
    """from the cases' own numbers (allocations are aligned to 16 bytes at least)"""
    last_halved = lambda n: len(CASES[n][0]) - 1 in CASES[n][3]
    assert {d for n, d, _ in RUNS if not last_halved(n)} == {F64, F32}                 # the kept form along the contiguous axis
    seen = {F64: set(), F32: set()}
    for name, dtype, offset in RUNS:
        fbox, flo, fm, axes, _ = CASES[name]
        if not last_halved(name):
            continue
        size = np.dtype(dtype).itemsize
        rows = int(np.prod(fbox[:-1])) if len(fbox) > 1 else 1
        starts = {(offset + (r * fbox[-1] + flo[-1]) * size) % (2 * size) == 0 for r in range(min(rows, 4))}
        seen[dtype].add("mixed" if len(starts) == 2 else "aligned" if True in starts else "misaligned")
    assert seen[F64] == seen[F32] == {"aligned", "misaligned", "mixed"}, seen           # both forms of the pair load
    halved_rows = [_coarse(n)[-1] for n in CASES if last_halved(n)]
    # wave-edge lanes: lane 63 of a wave with a successor cell and lane 0 of a wave with a predecessor, inside one workgroup
    assert any(64 < m for m in halved_rows)
    # ... and across a chunk boundary inside a row, with a tail that is no multiple of a wave
    assert any(m > 256 and m % 64 for m in halved_rows)
    # a row shorter than a wave, whose last lanes own no cell, and one that ends on lane 0 of a wave (m % 64 == 1)
    assert any(m < 64 for m in halved_rows) and any(m % 64 == 1 for m in halved_rows)
    # a run boundary inside a plane (axis 1 halved and more coarse rows than one run), a last run that is short, and planes of
    # a single run
    marched = [_coarse(n)[-2] for n in CASES if len(CASES[n][0]) >= 2 and len(CASES[n][0]) - 2 in CASES[n][3]]
    assert any(m > 2 * RUN and m % RUN for m in marched) and any(m < RUN for m in marched)
    # both ghost ends on every axis, on separate coarse cells (m_c >= 2) and on the same one (m_c = 1)
    for axis in range(3):
        extents = [_coarse(n)[d] for n in CASES for d in CASES[n][3] if d + 3 - len(CASES[n][0]) == axis]
        assert any(m >= 2 for m in extents), axis
    assert any(_coarse(n)[d] == 1 for n in CASES for d in CASES[n][3])
    # every face meets both rules: a pattern and its complement
    for name in CASES:
        assert all({a, b} == {EVEN, ODD} for p, q in zip(_rim(name, False), _rim(name, True)) for a, b in zip(p, q))


@pytest.fixture(scope="module")
def nh(built_libs):
    ns = mg_device.namespace()
    assert hasattr(ns.lib, "neptune_hip_mg_restrict_linear")
    return ns


RSCALE = 3.0                                       # not a power of two: the last operation rounds


def Geometry(nh, name, dtype, rim=None):
    fbox, flo, fm, axes, clo = CASES[name]
    cm = _coarse(name)
    setting = {} if rim is None else dict(restrict="linear", faces=rst.faces_of(rim))
    return mg_device.Geometry(nh, (fbox, flo, fm), (mg_device.unequal_rims(clo, cm), clo, cm), dtype, axes, rscale=RSCALE, **setting)


def field(shape, dtype, seed, where):
    """hashed values with -0 sprinkled in on `where`, NaN on every other cell"""
    return mg_device.field(shape, dtype, seed, where, np.nan)


def _inputs(G, dtype):
    b_f, q_f = field(G.fine_shape, dtype, 51, G.fw), field(G.fine_shape, dtype, 52, G.fw)      # NaN outside the fine Omega
    b_c, x_c = helpers.hash_field(G.coarse_shape, dtype, seed=53), helpers.hash_field(G.coarse_shape, dtype, seed=54)
    q_f[q_f == 0] = 0.0                                       # q's zeros are +0, so that d = -0 - +0 = -0 where b is -0
    d = b_f[G.fw] - q_f[G.fw]
    assert np.isfinite(d).all() and np.signbit(d[d == 0]).any()
    return b_f, q_f, b_c, x_c


def _run(nh, name, dtype, offset, complemented):
    rim = _rim(name, complemented)
    G = Geometry(nh, name, dtype, rim)
    assert nh.mg.halved_axes(G.fine, G.coarse) == G.axes
    b_f, q_f, b_c, x_c = _inputs(G, dtype)
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, RSCALE, b_c, x_c, G.cw, Transfers(G.axes, rim))
    bd, xd = dev(nh, b_c, offset), dev(nh, x_c, offset)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, offset), dev(nh, q_f, offset), bd, xd)
    nh.torch.cuda.synchronize()
    got_b, got_x = bd.numpy(), xd.numpy()
    assert bits_equal(got_b, want_b), mismatch_report(got_b, want_b)
    assert bits_equal(got_x, want_x), mismatch_report(got_x, want_x)
    assert np.isfinite(got_b).all()                                                    # no fine cell outside Omega was read
    outside = np.ones(G.coarse_shape, bool)
    outside[G.cw] = False
    assert bits_equal(got_b[outside], b_c[outside]) and bits_equal(got_x[outside], x_c[outside])
    assert (got_x[G.cw] == 0).all() and not np.signbit(got_x[G.cw]).any()


@pytest.mark.parametrize("complemented", [False, True], ids=["rules", "complement"])
@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS(RUNS))
def test_restrict_linear(nh, name, dtype, offset, complemented):
    _run(nh, name, dtype, offset, complemented)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_minus_zero_and_the_exact_sign_flip(nh, dtype):
    """d = -0 everywhere (b = -0, q = +0): a coarse cell on an ODD face gets +0 (its ghost is -(-0) = +0 and +0 + -0 = +0), every
    other one -0, and rscale keeps the sign.  One fine spike of 64 in an ODD low corner comes out as 64 * (1/4)^3 in the corner
    cell -- the ghosts of the later dimensions are the intermediates' own"""
    rim = ((ODD, EVEN), (ODD, EVEN), (ODD, EVEN))
    G = Geometry(nh, "r3-012", dtype, rim)
    b_f, q_f = np.full(G.fine_shape, np.nan, dtype), np.full(G.fine_shape, np.nan, dtype)
    b_f[G.fw], q_f[G.fw] = -0.0, 0.0
    ones = np.ones(G.coarse_shape, dtype)
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, RSCALE, ones, ones, G.cw, Transfers(G.axes, rim))
    bd, xd = dev(nh, ones, 0), dev(nh, ones, 0)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, 0), dev(nh, q_f, 0), bd, xd)
    nh.torch.cuda.synchronize()
    got = bd.numpy()
    assert bits_equal(got, want_b), mismatch_report(got, want_b)
    assert bits_equal(xd.numpy(), want_x)
    inner = got[G.cw]
    assert (inner == 0).all()
    on_odd_face = np.zeros(inner.shape, bool)
    on_odd_face[0], on_odd_face[:, 0], on_odd_face[:, :, 0] = True, True, True
    assert not np.signbit(inner[on_odd_face]).any() and np.signbit(inner[~on_odd_face]).all()
    b_f[G.fw] = 0.0
    b_f[G.fw[0].start, G.fw[1].start, G.fw[2].start] = 64.0
    bd = dev(nh, ones, 0)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, 0), dev(nh, q_f, 0), bd, dev(nh, ones, 0))
    nh.torch.cuda.synchronize()
    inner = bd.numpy()[G.cw]
    assert inner[0, 0, 0] == RSCALE * 64.0 * 0.25 ** 3 and (inner.reshape(-1)[1:] == 0).all()


def _transfer(nh, prolong, restrict, lo=(0, 0, 0), hi=(0, 0, 0)):
    t = nh.capi.MgTransfer()
    t.prolong, t.restrict_kind = prolong, restrict
    for d in range(3):
        t.rim_lo[d], t.rim_hi[d] = lo[d], hi[d]
    return t


@pytest.mark.parametrize("name", ["r3-012", "r2-1", "r3-01"])
def test_kind_average_is_the_averaging_restriction(nh, name):
    """through neptune_hip_mg_restrict_linear: restrict_kind AVERAGE is neptune_hip_mg_restrict's bits whatever the rules and
    the prolongation's kind hold (the rules of such an entry are not read); on a rank-2 pair the rules of dimension 2 are not
    read"""
    lib, f64 = nh.lib, nh.capi.F64
    G = Geometry(nh, name, F64)
    b_f, q_f, b_c, x_c = _inputs(G, F64)
    t = _transfer(nh, nh.capi.MG_PROLONG_CONSTANT, nh.capi.MG_RESTRICT_AVERAGE, (9, 9, 9), (-9, -9, -9))
    bd, xd = dev(nh, b_c, 0), dev(nh, x_c, 0)
    assert lib.neptune_hip_mg_restrict_linear(f64, C.byref(G.fine.geom), C.byref(G.coarse.geom), C.byref(t), dev(nh, b_f, 0).ptr,
                                              dev(nh, q_f, 0).ptr, RSCALE, bd.ptr, xd.ptr, None) == nh.capi.OK
    b2, x2 = dev(nh, b_c, 0), dev(nh, x_c, 0)
    assert lib.neptune_hip_mg_restrict(f64, C.byref(G.fine.geom), C.byref(G.coarse.geom), dev(nh, b_f, 0).ptr, dev(nh, q_f, 0).ptr,
                                       RSCALE, b2.ptr, x2.ptr, None) == nh.capi.OK
    nh.torch.cuda.synchronize()
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, RSCALE, b_c, x_c, G.cw, Halved(G.axes))
    assert bits_equal(bd.numpy(), b2.numpy()) and bits_equal(xd.numpy(), x2.numpy())
    assert bits_equal(bd.numpy(), want_b), mismatch_report(bd.numpy(), want_b)
    assert bits_equal(xd.numpy(), want_x)
    if len(G.fine_shape) == 2:
        t = _transfer(nh, nh.capi.MG_PROLONG_CONSTANT, nh.capi.MG_RESTRICT_LINEAR, (ODD, EVEN, 9), (EVEN, ODD, -9))
        bd, xd = dev(nh, b_c, 0), dev(nh, x_c, 0)
        assert lib.neptune_hip_mg_restrict_linear(f64, C.byref(G.fine.geom), C.byref(G.coarse.geom), C.byref(t), dev(nh, b_f, 0).ptr,
                                                  dev(nh, q_f, 0).ptr, RSCALE, bd.ptr, xd.ptr, None) == nh.capi.OK
        nh.torch.cuda.synchronize()
        want_b, _ = rst.restrict(b_f, q_f, G.fw, RSCALE, b_c, x_c, G.cw, Transfers(G.axes, ((ODD, EVEN), (EVEN, ODD))))
        assert bits_equal(bd.numpy(), want_b), mismatch_report(bd.numpy(), want_b)


def test_refusals_on_device_pointers(nh):
    G = Geometry(nh, "r3-012", np.float64)
    F = nh.fields.DeviceField
    bf, qf = F.from_numpy(np.full(G.fine_shape, 3.0)), F.from_numpy(np.full(G.fine_shape, 2.0))
    bc, xc = F.from_numpy(np.full(G.coarse_shape, 5.0)), F.from_numpy(np.full(G.coarse_shape, 6.0))
    lib, E, f64 = nh.lib, nh.capi.EINVAL, nh.capi.F64
    lin, avg, const = nh.capi.MG_RESTRICT_LINEAR, nh.capi.MG_RESTRICT_AVERAGE, nh.capi.MG_PROLONG_CONSTANT
    gf, gc = G.fine.geom, G.coarse.geom
    call = lambda t, g_fine=gf, g_coarse=gc, b_coarse=bc, x_coarse=xc, rscale=4.0: lib.neptune_hip_mg_restrict_linear(
        f64, C.byref(g_fine), C.byref(g_coarse), C.byref(t) if t is not None else None, bf.ptr, qf.ptr, rscale, b_coarse.ptr, x_coarse.ptr,
        None)
    assert call(None) == E
    assert call(_transfer(nh, const, 2)) == E and call(_transfer(nh, const, -1)) == E and call(_transfer(nh, 2, lin)) == E
    for d in range(3):
        lo, hi = [0, 0, 0], [1, 1, 1]
        lo[d] = 2
        assert call(_transfer(nh, const, lin, lo, hi)) == E
        lo[d], hi[d] = 0, -1
        assert call(_transfer(nh, const, lin, lo, hi)) == E
    # LINEAR on a vertex-centred pair: fine Omega 7 x 15 x 263 onto 3 x 7 x 131
    like_f = F.from_numpy(np.zeros(G.fine_shape))
    vertex = nh.mg.Level(None, like_f, ([1, 2, 3], [8, 17, 266])).geom
    assert call(_transfer(nh, const, lin), g_fine=vertex) == E
    assert call(_transfer(nh, const, lin), g_fine=gc, g_coarse=gf) == E                # the wrong way round
    assert call(_transfer(nh, const, lin), b_coarse=bf) == E                           # a written field overlaps a read one
    assert call(_transfer(nh, const, lin), x_coarse=bc) == E                           # the two written fields overlap
    assert call(_transfer(nh, const, lin), rscale=float("nan")) == E
    nh.torch.cuda.synchronize()
    for f, v in ((bf, 3.0), (qf, 2.0), (bc, 5.0), (xc, 6.0)):
        assert bool((f.tensor == v).all())
    with pytest.raises(nh.capi.NeptuneHipError):
        bad = Geometry(nh, "r3-012", np.float64, ((EVEN, EVEN),) * 3)
        bad.fine.geom = vertex
        nh.mg.restrict(bad.fine, bad.coarse, bf, qf, bc, xc)
    # ... and accepted as it stands
    assert call(_transfer(nh, const, lin, (1, 0, 1), (0, 1, 0))) == nh.capi.OK
    nh.torch.cuda.synchronize()
    assert bool((bc.tensor[G.cw] != 5.0).all()) and bool((xc.tensor[G.cw] == 0.0).all())
