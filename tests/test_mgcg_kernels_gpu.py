"""neptune_hip_mg_smooth_dot alone against the NumPy restatement: x bit for bit on every cell, the untouched
cells outside Omega included (mg_restatement.smooth), and the sum of b * x_new over Omega within 2 (n - 1) eps sum |t_i| of the
exact sum of the restatement's own terms (cg_cases.dot_terms).

Shapes: those of tests/test_mg_kernels_gpu.py -- fine box 9 x 18 x 268 with Omega 7 x 15 x 263 at (1, 2, 3): unequal rims, a
row that crosses the 256-cell chunk with an odd tail (two workgroups per row, one of them with 7 cells), more than one
partial -- in ranks 3, 2 and 1, both element types, and with the fields 8 bytes into larger allocations.  The inputs hold -0
in places and NaN on every cell outside Omega, which the definition says is never read."""
import numpy as np
import pytest

import cg_cases as cc
import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import dev, field

pytestmark = pytest.mark.gpu

# name: (box, Omega lower corner, Omega extents)
CASES = {
    "rank3": ((9, 18, 268), (1, 2, 3), (7, 15, 263)),
    "rank2": ((17, 266), (1, 2), (15, 263)),
    "rank1": ((267,), (3,), (263,)),
}
RUNS = [("rank3", np.float64, 0), ("rank3", np.float32, 0), ("rank2", np.float64, 0), ("rank2", np.float32, 0),
        ("rank1", np.float64, 0), ("rank1", np.float32, 0), ("rank3", np.float64, 8), ("rank3", np.float32, 8)]
IDS = [f"{n}-{np.dtype(d).name}" + ("-offset" if o else "") for n, d, o in RUNS]


@pytest.fixture(scope="module")
def nh(built_libs):
    return mg_device.namespace()


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_smooth_dot(nh, name, dtype, offset):
    box, lo, m = CASES[name]
    w = tuple(slice(l, l + n) for l, n in zip(lo, m))
    q = field(box, dtype, 11, w, np.nan)
    b = field(box, dtype, 12, w, np.nan)
    minv = field(box, dtype, 13, w, np.nan)
    x = field(box, dtype, 14)
    x[tuple(0 for _ in box)] = np.nan          # a NaN and a -0 outside Omega keep their bits
    x[tuple(n - 1 for n in box)] = -0.0
    want = rst.smooth(q, b, minv, x, w)
    want_sum, bound = cc.dot_terms(b, want, w)
    level = nh.mg.Level(None, nh.fields.DeviceField.from_numpy(np.zeros(box, dtype)), ([s.start for s in w], [s.stop for s in w]))
    level.minv = dev(nh, minv, offset)
    xd = dev(nh, x, offset)
    # the sum lands in the second of three elements: its neighbours keep their values
    out = nh.torch.full((3,), -7.0, dtype=xd.tensor.dtype, device="cuda")
    assert nh.mg.smooth_dot(level, dev(nh, q, offset), dev(nh, b, offset), xd, dot_out=out[1:2]) is None
    nh.torch.cuda.synchronize()
    got, sums = xd.numpy(), out.cpu().numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    print(f"{name} {np.dtype(dtype).name}: sum = {float(sums[1])!r} (terms' sum {want_sum!r}, bound {bound:.3e})")
    assert sums[0] == -7.0 and sums[2] == -7.0
    assert np.isfinite(sums[1]) and abs(float(sums[1]) - want_sum) <= bound
    # the blocking form returns the same sum, bit for bit (one fixed tree), from the same start
    xd2 = dev(nh, x, offset)
    again = nh.mg.smooth_dot(level, dev(nh, q, offset), dev(nh, b, offset), xd2)
    assert again == float(sums[1]) and bits_equal(xd2.numpy(), want)


def test_smooth_dot_refusals_on_device_pointers(nh):
    box, lo, m = CASES["rank3"]
    w = tuple(slice(l, l + n) for l, n in zip(lo, m))
    F = nh.fields.DeviceField
    level = nh.mg.Level(None, F.from_numpy(np.zeros(box)), ([s.start for s in w], [s.stop for s in w]))
    q, b, minv, x = (F.from_numpy(np.full(box, v)) for v in (1.0, 2.0, 3.0, 4.0))
    out = nh.torch.full((1,), -7.0, dtype=nh.torch.float64, device="cuda")
    import ctypes as C
    g = C.byref(level.geom)
    E = nh.capi.EINVAL
    call = lambda *a: nh.lib.neptune_hip_mg_smooth_dot(nh.capi.F64, g, *a, None)
    n_bytes = int(np.prod(box)) * 8
    assert call(q.ptr, b.ptr, minv.ptr, x.ptr, None) == E
    for f in (q, b, minv, x):
        assert call(q.ptr, b.ptr, minv.ptr, x.ptr, f.ptr) == E
        assert call(q.ptr, b.ptr, minv.ptr, x.ptr, f.ptr + n_bytes - 8) == E
    assert call(x.ptr, b.ptr, minv.ptr, x.ptr, out.data_ptr()) == E
    assert call(q.ptr, b.ptr, minv.ptr, x.ptr, out.data_ptr() + 4) == E
    nh.torch.cuda.synchronize()
    assert float(out[0]) == -7.0 and bool((x.tensor == 4.0).all()) and bool((q.tensor == 1.0).all())
