"""The three multigrid kernels alone (neptune_hip_mg_smooth / _restrict / _prolong_add) against the NumPy
restatement of tests/mg_restatement.py: bit for bit on every cell, the untouched cells outside Omega included.

Shapes: the smallest at which the kernels can go wrong -- unequal rims, a row that crosses the 256-cell chunk with an odd
tail, ranks 1 to 3, fields 8 bytes into larger allocations (the unaligned forms), and a coarse grid one cell thick, where
every even fine plane interpolates against the +0 rim on both sides.  The inputs hold -0 in places, NaN on every cell
outside Omega that the definition says is never read, and minv is NaN outside Omega."""
import numpy as np
import pytest

import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import dev, field

pytestmark = pytest.mark.gpu

# name: (fine box, fine Omega lower corner, fine Omega extents, coarse box, coarse Omega lower corner)
CASES = {
    "rank3": ((9, 18, 268), (1, 2, 3), (7, 15, 263), (5, 9, 135), (1, 1, 2)),
    "rank2": ((17, 266), (1, 2), (15, 263), (9, 134), (1, 2)),
    "rank1": ((267,), (3,), (263,), (134,), (2,)),
    "thin": ((5, 9, 135), (1, 1, 2), (3, 7, 131), (3, 5, 67), (1, 1, 1)),          # coarse Omega 1 x 3 x 65
}
RUNS = [("rank3", np.float64, 0), ("rank3", np.float32, 0), ("rank2", np.float64, 0), ("rank2", np.float32, 0),
        ("rank1", np.float64, 0), ("rank1", np.float32, 0), ("rank3", np.float64, 8), ("rank3", np.float32, 8),
        ("thin", np.float64, 0), ("thin", np.float32, 0)]
IDS = [f"{n}-{np.dtype(d).name}" + ("-offset" if o else "") for n, d, o in RUNS]


@pytest.fixture(scope="module")
def nh(built_libs):
    return mg_device.namespace()


def Geometry(nh, name, dtype):
    fbox, flo, fm, cbox, clo = CASES[name]
    cm = tuple((m - 1) // 2 for m in fm)
    return mg_device.Geometry(nh, (fbox, flo, fm), (cbox, clo, cm), dtype)


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_smooth(nh, name, dtype, offset):
    G = Geometry(nh, name, dtype)
    shape, w = G.fine_shape, G.fw
    q = field(shape, dtype, 11, w, np.nan)
    b = field(shape, dtype, 12, w, np.nan)
    minv = field(shape, dtype, 13, w, np.nan)
    x = field(shape, dtype, 14)
    x[tuple(0 for _ in shape)] = np.nan          # a NaN and a -0 outside Omega keep their bits
    x[tuple(n - 1 for n in shape)] = -0.0
    want = rst.smooth(q, b, minv, x, w)
    G.fine.minv = dev(nh, minv, offset)
    xd = dev(nh, x, offset)
    nh.mg.smooth(G.fine, dev(nh, q, offset), dev(nh, b, offset), xd)
    nh.torch.cuda.synchronize()
    got = xd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_restrict(nh, name, dtype, offset):
    G = Geometry(nh, name, dtype)
    b_f = field(G.fine_shape, dtype, 21, G.fw, np.nan)       # nothing outside the fine Omega is read
    q_f = field(G.fine_shape, dtype, 22, G.fw, np.nan)
    b_c = field(G.coarse_shape, dtype, 23)
    x_c = field(G.coarse_shape, dtype, 24)
    for a in (b_c, x_c):
        a[tuple(0 for _ in a.shape)] = np.nan
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, rst.RSCALE, b_c, x_c, G.cw)
    bd, xd = dev(nh, b_c, offset), dev(nh, x_c, offset)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, offset), dev(nh, q_f, offset), bd, xd)
    nh.torch.cuda.synchronize()
    got_b, got_x = bd.numpy(), xd.numpy()
    assert bits_equal(got_b, want_b), mismatch_report(got_b, want_b)
    assert bits_equal(got_x, want_x), mismatch_report(got_x, want_x)
    assert not np.signbit(got_x[G.cw]).any()


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_prolong_add(nh, name, dtype, offset):
    G = Geometry(nh, name, dtype)
    x_c = field(G.coarse_shape, dtype, 31, G.cw, np.nan)     # the coarse rim is +0 whatever the field holds there
    x_f = field(G.fine_shape, dtype, 32)
    x_f[tuple(0 for _ in x_f.shape)] = np.nan
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw)
    xd = dev(nh, x_f, offset)
    nh.mg.prolong_add(G.fine, G.coarse, dev(nh, x_c, offset), xd)
    nh.torch.cuda.synchronize()
    got = xd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    assert np.isfinite(got[G.fw]).all()
