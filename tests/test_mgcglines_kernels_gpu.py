"""The two further forms of the line stage's kernel alone (neptune_hip_mg_line_first, neptune_hip_mg_line_smooth_dot; DESIGN
3.18) against the NumPy restatement of tests/mg_restatement.py: bit for bit on every cell of x,
the untouched cells outside Omega included, and q outside Omega; *dot_out within cg_cases.dot_terms' bound -- 2 (n - 1) eps
sum |t_i|, what two summation orders may differ by -- of the exact sum of its own terms b * x_new.

Shapes: those of tests/test_mglines_kernels_gpu.py, for the same reasons.  Box 9 x 18 x 268 with Omega 7 x 15 x 263 at
(1, 2, 3) along each axis (contiguous-axis lines cross every 32-cell segment and end in a 7-cell tail, 105 lines = one full
group of 64 and a tail of 41, slow-axis chunks cross the 64-lane workgroup with a 7-lane tail); Omega 3 x 257 x 263 along dim 0
and 257 x 3 x 263 along dim 1 (256-lane workgroups: four waves per partial, an odd tail of 7 lanes whose waves add +0);
131 x 3 x 65 along dim 0 (64-lane workgroups, a long line past the unroll's tail); m[a] = 1 and 2 for a slow and for the
contiguous axis; rank 2 both axes; rank 1.  f64 and f32; every field 8 bytes into a larger allocation.

The inputs hold -0 in places and NaN on every cell the definition says is not read: lo at i = 0, up at i = m - 1, the factor
fields, b and q outside Omega -- and, for the apply-free stage, x on Omega."""
import ctypes as C

import numpy as np
import pytest

import cg_cases as cc
import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import level as _level, outside_of as _outside

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
def test_apply_free_stage_matches_the_restatement_and_the_plain_kernel(nh, name, axis, dtype):
    where, q, b, x, (lo, inv, up) = _problem(name, axis, dtype)
    x_nan = x.copy()
    x_nan[where] = np.nan                                             # the stage must not read x on Omega
    want = rst.first_stage(b, lo, inv, up, x_nan, where, axis)
    assert np.isfinite(want[where]).all()
    dev = lambda a: mg_device.dev(nh, a, 8)                           # every field 8 bytes into a larger allocation
    level = _level(nh, x.shape, dtype, where)
    stage = nh.mg.LineStage(axis, dev(lo), dev(inv), dev(up))
    bd, xd = dev(b), dev(x_nan)
    nh.mg.line_first(level, stage, bd, xd)
    # the plain kernel on zero-filled q and x
    zero_on_omega = lambda a: np.where(_outside(a.shape, where), a, 0).astype(dtype)
    qz, xz = dev(zero_on_omega(q)), dev(zero_on_omega(x))
    nh.mg.line_smooth(level, stage, qz, bd, xz)
    nh.torch.cuda.synchronize()
    got, plain = xd.numpy(), xz.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    assert bits_equal(got[where], plain[where]), mismatch_report(got[where], plain[where])
    assert bd.numpy().tobytes() == b.tobytes()


@pytest.mark.parametrize("name,axis,dtype", RUNS, ids=IDS)
def test_stage_with_a_sum_matches_the_restatement(nh, name, axis, dtype):
    where, q, b, x, (lo, inv, up) = _problem(name, axis, dtype)
    want = rst.line_stage(q, b, lo, inv, up, x, where, axis)
    assert np.isfinite(want[where]).all()
    total, bound = cc.dot_terms(b, want, where)
    dev = lambda a: mg_device.dev(nh, a, 8)
    level = _level(nh, x.shape, dtype, where)
    stage = nh.mg.LineStage(axis, dev(lo), dev(inv), dev(up))
    qd, xd = dev(q), dev(x)
    out = nh.torch.full((3,), float("nan"), dtype=xd.tensor.dtype, device=xd.tensor.device)
    assert nh.mg.line_smooth_dot(level, stage, qd, dev(b), xd, dot_out=out[1:2]) is None
    nh.torch.cuda.synchronize()
    got, got_q, sums = xd.numpy(), qd.numpy(), out.cpu().numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    outside = _outside(x.shape, where)
    assert got_q[outside].tobytes() == q[outside].tobytes()          # q keeps its bits outside Omega
    print(f"dot = {float(sums[1])!r} (terms' sum {total!r}, bound {bound:.3e})")
    assert np.isnan(sums[0]) and np.isnan(sums[2])                   # one T is written
    assert abs(float(sums[1]) - total) <= bound
    # the blocking form returns the same sum, bit for bit: the order of the additions is fixed
    qd, xd = dev(q), dev(x)
    again = nh.mg.line_smooth_dot(level, stage, qd, dev(b), xd)
    assert again == float(sums[1]) and bits_equal(xd.numpy(), want)


def test_refusals_on_device_pointers(nh):
    box, lo_corner, om = MAIN
    where = tuple(slice(l, l + m) for l, m in zip(lo_corner, om))
    F = nh.fields.DeviceField
    q, b, lo, inv, up, x = (F.from_numpy(np.full(box, float(v))) for v in range(1, 7))
    dot = nh.torch.full((2,), 9.0, dtype=nh.torch.float64, device=x.tensor.device)
    d = dot.data_ptr()
    level = nh.mg.Level(None, x, ([s.start for s in where], [s.stop for s in where]))
    lib, E, f64 = nh.lib, nh.capi.EINVAL, nh.capi.F64
    g = C.byref(level.geom)
    rank2 = nh.mg.Level(None, F.from_numpy(np.zeros((17, 266))), ([1, 2], [16, 265]))
    n_bytes = int(np.prod(box)) * 8

    good = [b.ptr, lo.ptr, inv.ptr, up.ptr, x.ptr]
    first = lib.neptune_hip_mg_line_first
    for axis in (-1, 3):
        assert first(f64, g, axis, *good, None) == E
    assert first(5, g, 0, *good, None) == E and first(f64, C.byref(rank2.geom), 2, *good, None) == E
    for k in range(5):
        args = list(good)
        args[k] = None
        assert first(f64, g, 2, *args, None) == E, k
    for k in range(4):
        args = list(good)
        args[k] = x.ptr
        assert first(f64, g, 1, *args, None) == E, k

    good = [q.ptr, b.ptr, lo.ptr, inv.ptr, up.ptr, x.ptr]
    sdot = lib.neptune_hip_mg_line_smooth_dot
    for axis in (-1, 3):
        assert sdot(f64, g, axis, *good, d, None) == E
    assert sdot(5, g, 0, *good, d, None) == E and sdot(f64, C.byref(rank2.geom), 2, *good, d, None) == E
    for k in range(6):
        args = list(good)
        args[k] = None
        assert sdot(f64, g, 2, *args, d, None) == E, k
    for k in range(5):
        args = list(good)
        args[k] = x.ptr
        assert sdot(f64, g, 1, *args, d, None) == E, k
    for k in range(1, 5):
        args = list(good)
        args[k] = q.ptr + 8
        assert sdot(f64, g, 1, *args, d, None) == E, k
    assert sdot(f64, g, 1, *good, None, None) == E and sdot(f64, g, 1, *good, d + 4, None) == E
    for p in good:
        assert sdot(f64, g, 1, *good, p, None) == E and sdot(f64, g, 1, *good, p + n_bytes - 8, None) == E
    nh.torch.cuda.synchronize()
    for v, f in enumerate((q, b, lo, inv, up, x), start=1):
        assert bool((f.tensor == float(v)).all())
    assert bool((dot == 9.0).all())
