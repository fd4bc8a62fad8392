"""The line stage's kernels alone (neptune_hip_mg_line_smooth) against the NumPy restatement of
tests/mg_restatement.py: bit for bit on every cell of x, the untouched cells outside Omega included, and q outside Omega.

Shapes: the smallest at which the kernels can go wrong.  Box 9 x 18 x 268 with Omega 7 x 15 x 263 at (1, 2, 3), lines along
each axis: contiguous-axis lines of 263 cells cross every 32-cell segment boundary and end in a 7-cell tail, there are 105 of
them (one full group of 64 and a tail of 41), and the slow-axis chunks cross the 64-lane workgroup with a 7-lane tail.  Omega
3 x 257 x 263 along dim 0 and 257 x 3 x 263 along dim 1 have enough lines for the 256-lane workgroups (on the 256 CUs of
an MI355X): chunks of 256 and an odd tail of 7.  Omega 131 x 3 x 65 along dim 0: a long slow-axis line, 130 = 4 * 32 + 2 steps
past the unroll's tail in both directions.  m[a] = 1 and 2 for a slow and for the contiguous axis.  Rank 2, 15 x 263, both
axes; rank 1, one single line of 263.  f64 and f32; every field 8 bytes into a larger allocation.

The inputs hold -0 in places and NaN on every cell the definition says is not read: lo at i = 0, up at i = m - 1, and the
factor fields, b and q outside Omega.  The factor fields come from the restatement's recurrence on the host, on a random
diagonally dominant T."""
import ctypes as C

import numpy as np
import pytest

import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

MAIN = ((9, 18, 268), (1, 2, 3), (7, 15, 263))
# name: (box, Omega's lower corner, Omega, the axes to run)
CASES = {
    "main": MAIN + ((0, 1, 2),),
    "wide-0": ((5, 259, 266), (1, 1, 2), (3, 257, 263), (0,)),
    "wide-1": ((259, 5, 266), (1, 1, 2), (257, 3, 263), (1,)),
    "long-0": ((133, 5, 68), (1, 1, 2), (131, 3, 65), (0,)),
    "one-slow": ((3, 17, 266), (1, 1, 2), (1, 15, 263), (0,)),
    "two-slow": ((9, 4, 266), (1, 1, 2), (7, 2, 263), (1,)),
    "one-contig": ((9, 17, 3), (1, 1, 1), (7, 15, 1), (2,)),
    "two-contig": ((9, 17, 5), (1, 1, 2), (7, 15, 2), (2,)),
    "rank2": ((17, 266), (1, 2), (15, 263), (0, 1)),
    "rank1": ((268,), (3,), (263,), (0,)),
}
RUNS = [(n, a, d) for n, c in CASES.items() for a in c[3] for d in (np.float64, np.float32)]
IDS = [f"{n}-axis{a}-{np.dtype(d).name}" for n, a, d in RUNS]


@pytest.fixture(scope="module")
def nh(built_libs):
    return mg_device.namespace()


def _problem(name, axis, dtype):
    return mg_device.line_problem(*CASES[name][:3], axis, dtype)


@pytest.mark.parametrize("name,axis,dtype", RUNS, ids=IDS)
def test_line_stage_matches_the_restatement(nh, name, axis, dtype):
    where, q, b, x, (lo, inv, up) = _problem(name, axis, dtype)
    want = rst.line_stage(q, b, lo, inv, up, x, where, axis)
    assert np.isfinite(want[where]).all()
    F = nh.fields.DeviceField
    dev = lambda a: mg_device.dev(nh, a, 8)                           # every field 8 bytes into a larger allocation
    level = nh.mg.Level(None, F.from_numpy(np.zeros(x.shape, dtype)), ([s.start for s in where], [s.stop for s in where]))
    qd, xd = dev(q), dev(x)
    stage = nh.mg.LineStage(axis, dev(lo), dev(inv), dev(up))
    nh.mg.line_smooth(level, stage, qd, dev(b), xd)
    nh.torch.cuda.synchronize()
    got, got_q = xd.numpy(), qd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    outside = np.ones(x.shape, bool)
    outside[where] = False
    assert got_q[outside].tobytes() == q[outside].tobytes()          # q keeps its bits outside Omega


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_cell_lines_are_the_point_sweep(nh, dtype):
    """m = 1 along the stage's axis with inv = minv: the bits of neptune_hip_mg_smooth"""
    for name, axis in (("one-slow", 0), ("one-contig", 2)):
        where, q, b, x, (lo, inv, up) = _problem(name, axis, dtype)
        F = nh.fields.DeviceField
        level = nh.mg.Level(None, F.from_numpy(np.zeros(x.shape, dtype)), ([s.start for s in where], [s.stop for s in where]),
                            minv=F.from_numpy(inv))
        xs, xl = F.from_numpy(x), F.from_numpy(x)
        nh.mg.smooth(level, F.from_numpy(q), F.from_numpy(b), xs)
        nh.mg.line_smooth(level, nh.mg.LineStage(axis, F.from_numpy(lo), F.from_numpy(inv), F.from_numpy(up)), F.from_numpy(q),
                          F.from_numpy(b), xl)
        nh.torch.cuda.synchronize()
        assert bits_equal(xl.numpy(), xs.numpy()) and bits_equal(xs.numpy(), rst.smooth(q, b, inv, x, where))


def test_refusals_on_device_pointers(nh):
    box, lo_corner, om = MAIN
    where = tuple(slice(l, l + m) for l, m in zip(lo_corner, om))
    F = nh.fields.DeviceField
    q, b, lo, inv, up, x = (F.from_numpy(np.full(box, float(v))) for v in range(1, 7))
    level = nh.mg.Level(None, x, ([s.start for s in where], [s.stop for s in where]))
    lib, E, f64 = nh.lib, nh.capi.EINVAL, nh.capi.F64
    g = C.byref(level.geom)
    good = [q.ptr, b.ptr, lo.ptr, inv.ptr, up.ptr, x.ptr]
    for axis in (-1, 3):
        assert lib.neptune_hip_mg_line_smooth(f64, g, axis, *good, None) == E
    assert lib.neptune_hip_mg_line_smooth(5, g, 0, *good, None) == E
    for k in range(6):
        args = list(good)
        args[k] = None
        assert lib.neptune_hip_mg_line_smooth(f64, g, 2, *args, None) == E, k
    for k in range(5):
        args = list(good)
        args[k] = x.ptr
        assert lib.neptune_hip_mg_line_smooth(f64, g, 1, *args, None) == E, k
    for k in range(1, 5):
        args = list(good)
        args[k] = q.ptr + 8
        assert lib.neptune_hip_mg_line_smooth(f64, g, 1, *args, None) == E, k
    rank2 = nh.mg.Level(None, F.from_numpy(np.zeros((17, 266))), ([1, 2], [16, 265]))
    assert lib.neptune_hip_mg_line_smooth(f64, C.byref(rank2.geom), 2, *good, None) == E
    nh.torch.cuda.synchronize()
    for v, f in enumerate((q, b, lo, inv, up, x), start=1):
        assert bool((f.tensor == float(v)).all())
