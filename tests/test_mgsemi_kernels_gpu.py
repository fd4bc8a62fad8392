"""The two transfer kernels on semi-coarsened level pairs (neptune_hip_mg_restrict / _prolong_add) against the
NumPy restatement of tests/mg_restatement.py: each kernel alone, bit for bit on every cell, the untouched cells outside Omega
included.

Shapes: the smallest at which the kernels can go wrong.  Rank 3: fine box 9 x 18 x 268 with Omega 7 x 15 x 263 at (1, 2, 3)
under each of the six partial masks -- the kept 263-cell row crosses the 256-cell chunk with a 7-cell tail, the coarsened
one has 131 cells.  Omega 3 x 3 x 1031 with only the contiguous axis coarsened: 515 coarse cells, two full chunks and a
3-cell tail, staged segments of 513, 513 and the rest.  Rank 2: 15 x 263 under both partial masks.  A level one cell thick
along a kept axis (1 x 15 x 263 -> 1 x 7 x 131) and along a coarsened one (3 -> 1).  f64 and f32; fields 8 bytes into larger
allocations.  The inputs hold -0 in places and NaN on every cell the definition says is not read: outside the fine Omega for
the restriction, the coarse rim for the prolongation, the coarse b and x (on Omega) before the restriction."""
import ctypes as C

import numpy as np
import pytest

import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import dev, field

pytestmark = pytest.mark.gpu

R3 = ((9, 18, 268), (1, 2, 3), (7, 15, 263))      # fine box, fine Omega's lower corner, fine Omega
R2 = ((17, 266), (1, 2), (15, 263))
# name: (fine box, fine Omega's lower corner, fine Omega, the dimensions coarsened, coarse Omega's lower corner)
CASES = {
    "r3-0": R3 + ((0,), (1, 1, 2)), "r3-1": R3 + ((1,), (2, 1, 1)), "r3-2": R3 + ((2,), (1, 2, 1)),
    "r3-01": R3 + ((0, 1), (1, 1, 3)), "r3-02": R3 + ((0, 2), (1, 2, 2)), "r3-12": R3 + ((1, 2), (2, 1, 2)),
    "long-2": ((5, 5, 1035), (1, 1, 2), (3, 3, 1031), (2,), (1, 1, 1)),
    "r2-0": R2 + ((0,), (1, 2)), "r2-1": R2 + ((1,), (2, 1)),
    "thin-kept": ((3, 17, 266), (1, 1, 2), (1, 15, 263), (1, 2), (1, 1, 1)),
    "thin-coarsened": ((5, 17, 266), (1, 1, 2), (3, 15, 263), (0, 2), (1, 1, 1)),        # coarse Omega 1 x 15 x 131
}
RUNS = [(n, d, 0) for n in CASES for d in (np.float64, np.float32)] + \
       [(n, d, 8) for n in ("r3-0", "r3-1", "r3-2", "r3-01", "r3-02", "r3-12") for d in (np.float64, np.float32)]
IDS = [f"{n}-{np.dtype(d).name}" + ("-offset" if o else "") for n, d, o in RUNS]


@pytest.fixture(scope="module")
def nh(built_libs):
    return mg_device.namespace()


def Geometry(nh, name, dtype):
    fbox, flo, fm, axes, clo = CASES[name]
    cm = tuple((m - 1) // 2 if d in axes else m for d, m in enumerate(fm))
    return mg_device.Geometry(nh, (fbox, flo, fm), (mg_device.unequal_rims(clo, cm), clo, cm), dtype, axes)


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_restrict(nh, name, dtype, offset):
    G = Geometry(nh, name, dtype)
    assert nh.mg.coarsened_axes(G.fine, G.coarse) == G.axes
    b_f = field(G.fine_shape, dtype, 21, G.fw, np.nan)       # nothing outside the fine Omega is read
    q_f = field(G.fine_shape, dtype, 22, G.fw, np.nan)
    b_c = field(G.coarse_shape, dtype, 23, G.cw, inside=np.nan)      # what the coarse Omega held does not matter
    x_c = field(G.coarse_shape, dtype, 24, G.cw, inside=np.nan)
    for a in (b_c, x_c):
        a[tuple(0 for _ in a.shape)] = np.nan
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, 4.0, b_c, x_c, G.cw, G.axes)
    bd, xd = dev(nh, b_c, offset), dev(nh, x_c, offset)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, offset), dev(nh, q_f, offset), bd, xd)
    nh.torch.cuda.synchronize()
    got_b, got_x = bd.numpy(), xd.numpy()
    assert bits_equal(got_b, want_b), mismatch_report(got_b, want_b)
    assert bits_equal(got_x, want_x), mismatch_report(got_x, want_x)
    assert not np.signbit(got_x[G.cw]).any() and np.isfinite(got_b[G.cw]).all()


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_prolong_add(nh, name, dtype, offset):
    G = Geometry(nh, name, dtype)
    x_c = field(G.coarse_shape, dtype, 31, G.cw, np.nan)     # the coarse rim is +0 whatever the field holds there
    x_f = field(G.fine_shape, dtype, 32)
    x_f[tuple(0 for _ in x_f.shape)] = np.nan
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw, G.axes)
    xd = dev(nh, x_f, offset)
    nh.mg.prolong_add(G.fine, G.coarse, dev(nh, x_c, offset), xd)
    nh.torch.cuda.synchronize()
    got = xd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    assert np.isfinite(got[G.fw]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_kept_axis_hands_minus_zero_and_nan_through(nh, dtype):
    """axis 2 kept, axis 1 coarsened: a column of -0 and a column of NaN in d = b - q come out as -0 and NaN and touch no
    neighbouring column; prolongation adds the coarse -0 / NaN to the same column only"""
    G = Geometry(nh, "r3-1", dtype)
    G.fine.rscale = 1.0
    b_f = np.ones(G.fine_shape, dtype)
    q_f = np.zeros(G.fine_shape, dtype)
    k0, k1 = G.fw[2].start + 5, G.fw[2].start + 260
    b_f[:, :, k0] = -0.0
    b_f[:, :, k1] = np.nan
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, 1.0, np.zeros(G.coarse_shape, dtype), np.ones(G.coarse_shape, dtype), G.cw, G.axes)
    bd, xd = dev(nh, np.zeros(G.coarse_shape, dtype), 0), dev(nh, np.ones(G.coarse_shape, dtype), 0)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, 0), dev(nh, q_f, 0), bd, xd)
    nh.torch.cuda.synchronize()
    got = bd.numpy()
    assert bits_equal(got, want_b), mismatch_report(got, want_b)
    inner = got[G.cw]
    assert np.signbit(inner[:, :, 5]).all() and (inner[:, :, 5] == 0).all() and np.isnan(inner[:, :, 260]).all()
    assert np.isnan(inner).sum() == inner[:, :, 260].size and (np.delete(inner, [5, 260], axis=2) == 1).all()
    x_f = np.full(G.fine_shape, -0.0, dtype)
    want = rst.prolong_add(got, G.cw, x_f, G.fw, G.axes)
    fd = dev(nh, x_f, 0)
    nh.mg.prolong_add(G.fine, G.coarse, bd, fd)
    nh.torch.cuda.synchronize()
    out = fd.numpy()
    assert bits_equal(out, want), mismatch_report(out, want)
    # odd fine rows take the coarse value itself: -0 + -0 = -0
    assert np.signbit(out[G.fw][:, 1::2, 5]).all() and np.isnan(out[G.fw]).sum() == out[G.fw][:, :, 260].size


def test_refusals_on_device_pointers(nh):
    G = Geometry(nh, "r3-12", np.float64)
    F = nh.fields.DeviceField
    bf, qf, xf = (F.from_numpy(np.full(G.fine_shape, 3.0)) for _ in range(3))
    bc, xc = (F.from_numpy(np.full(G.coarse_shape, 5.0)) for _ in range(2))
    lib, E, f64 = nh.lib, nh.capi.EINVAL, nh.capi.F64
    gf = G.fine.geom
    like = F.from_numpy(np.zeros(G.coarse_shape))
    bad = []
    for lo, hi in (([2, 1, 2], [9, 8, 132]),        # dimension 2 is neither: 130 cells
                   ([2, 1, 2], [9, 9, 133]),        # dimension 1 is neither: 8 cells
                   ([2, 1, 2], [8, 8, 133])):       # dimension 0 is neither: 6 cells
        bad.append(nh.mg.Level(None, like, (lo, hi)).geom)
    for g in bad + [gf]:                            # ... and the all-kept pair
        assert lib.neptune_hip_mg_restrict(f64, C.byref(gf), C.byref(g), bf.ptr, qf.ptr, 4.0, bc.ptr, xc.ptr, None) == E
        assert lib.neptune_hip_mg_prolong_add(f64, C.byref(gf), C.byref(g), xc.ptr, xf.ptr, None) == E
        mask = C.c_int(-7)
        assert lib.neptune_hip_mg_coarsened_axes(C.byref(gf), C.byref(g), C.byref(mask)) == E and mask.value == -7
    gc = G.coarse.geom
    assert lib.neptune_hip_mg_restrict(f64, C.byref(gf), C.byref(gc), bf.ptr, qf.ptr, 4.0, bc.ptr, bc.ptr, None) == E
    assert lib.neptune_hip_mg_restrict(f64, C.byref(gf), C.byref(gc), bf.ptr, qf.ptr, float("inf"), bc.ptr, xc.ptr, None) == E
    assert lib.neptune_hip_mg_prolong_add(f64, C.byref(gf), C.byref(gc), xf.ptr, xf.ptr, None) == E
    assert lib.neptune_hip_mg_prolong_add(f64, C.byref(gc), C.byref(gf), xc.ptr, xf.ptr, None) == E       # the wrong way round
    nh.torch.cuda.synchronize()
    for f, v in ((bf, 3.0), (qf, 3.0), (xf, 3.0), (bc, 5.0), (xc, 5.0)):
        assert bool((f.tensor == v).all())
