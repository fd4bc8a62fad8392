"""The kernels at the seam of mixed-precision MGCG against the NumPy restatement.

neptune_hip_mg_smooth_dot_wide alone: x bit for bit the f32 sweep's -- the restatement's (mg_restatement.smooth) and the device's own
neptune_hip_mg_smooth --, the untouched cells outside Omega included, and the f64 sum of widen(b) * widen(x_new) over Omega
within 2 (n - 1) eps64 sum |t_i| of the exact sum of the restatement's own terms.  Shapes: Omega = 5 (a row shorter than a
wave), 9 x 70 (a wave and six lanes) and 3 x 5 x 300 (a row that crosses the 256-cell chunk: two workgroups per row, one with
44 cells) -- none a multiple of 256 --, in boxes with unequal rims.  The inputs hold -0 in places and NaN on every cell outside
Omega, which the definition says is never read.

The narrowing of the set-up (neptune_mgcg_init_mixed), run alone through a solve with max_iters = 0 from x = 0, so that
r = b on Omega: b holds exact ties between two f32 values in both directions, values that narrow into f32's subnormal
range, +-1e300 (which narrow to +-inf), -0 and NaN.  r must be b bit for bit on Omega and +0 outside, r32 must be
b.astype(float32), z32 must be minv_0 * r32, and rr_0 is NaN (or +inf without the NaN), as the restatement says."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_device
import mg_restatement as rst
import mgcgmixed_cases as mx
from helpers import bits_equal, mismatch_report
from mg_device import where_of as _where

pytestmark = pytest.mark.gpu

D, S = np.float64, np.float32
# name: (box, Omega lower corner, Omega extents)
CASES = {
    "rank1": ((9,), (3,), (5,)),
    "rank2": ((11, 75), (1, 2), (9, 70)),
    "rank3": ((5, 8, 304), (1, 2, 3), (3, 5, 300)),
}
# the set-up alone.  name: per level (box, Omega lower corner, Omega extents).  7 x 9 x 11: rows of 11 cells, every dimension
# coarsened; 3 x 300: a row of two chunks (256 + 44 cells of the box), Omega 1 x 297 with dim 0 kept (1 -> 1, 297 -> 148)
SETUPS = {
    "7x9x11": [((7, 9, 11), (1, 1, 1), (5, 7, 9)), ((4, 5, 6), (1, 1, 1), (2, 3, 4))],
    "3x300": [((3, 300), (1, 1), (1, 297)), ((3, 150), (1, 1), (1, 148))],
}


def _text(box, lo, m, dtype):
    return mgc.mc.star_module(box, dtype, bounds=(list(lo), [l + n for l, n in zip(lo, m)]), centre=float(2 * len(box)), side=-1.0)


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mg_device.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.setups = {}
    return ns


def _field(shape, seed, where=None, outside=None):
    """mg_device.field in f32"""
    return mg_device.field(shape, S, seed, where, outside)


# ---------------------------------------------------------------- neptune_hip_mg_smooth_dot_wide
@pytest.mark.parametrize("name", sorted(CASES))
def test_smooth_dot_wide(nh, name):
    box, lo, m = CASES[name]
    w = _where(lo, m)
    F = nh.fields.DeviceField
    q = _field(box, 11, w, np.nan)
    b = _field(box, 12, w, np.nan)
    minv = _field(box, 13, w, np.nan)
    x = _field(box, 14)
    x[tuple(0 for _ in box)] = np.nan          # a NaN and a -0 outside Omega keep their bits
    x[tuple(n - 1 for n in box)] = -0.0
    want = rst.smooth(q, b, minv, x, w)
    want_sum, bound = rst.wide_dot_terms(b, want, w)
    level = nh.mg.Level(None, F.from_numpy(np.zeros(box, S)), ([s.start for s in w], [s.stop for s in w]))
    level.minv = F.from_numpy(minv)
    # the f32 sweep alone, on the device
    plain = F.from_numpy(x)
    nh.mg.smooth(level, F.from_numpy(q), F.from_numpy(b), plain)
    xd = F.from_numpy(x)
    # the f64 sum lands in the second of three elements: its neighbours keep their values
    out = nh.torch.full((3,), -7.0, dtype=nh.torch.float64, device="cuda")
    assert nh.mg.smooth_dot_wide(level, F.from_numpy(q), F.from_numpy(b), xd, dot_out=out[1:2]) is None
    nh.torch.cuda.synchronize()
    got, sums = xd.numpy(), out.cpu().numpy()
    assert got.dtype == S and bits_equal(got, want), mismatch_report(got, want)
    assert bits_equal(got, plain.numpy())
    print(f"{name}: sum = {float(sums[1])!r} (terms' sum {want_sum!r}, bound {bound:.3e})")
    assert sums[0] == -7.0 and sums[2] == -7.0
    assert np.isfinite(sums[1]) and abs(float(sums[1]) - want_sum) <= bound
    # the blocking form returns the same sum, bit for bit (one fixed tree), from the same start
    xd2 = F.from_numpy(x)
    again = nh.mg.smooth_dot_wide(level, F.from_numpy(q), F.from_numpy(b), xd2)
    assert again == float(sums[1]) and bits_equal(xd2.numpy(), want)


def test_smooth_dot_wide_refusals_on_device_pointers(nh):
    box, lo, m = CASES["rank3"]
    w = _where(lo, m)
    F = nh.fields.DeviceField
    level = nh.mg.Level(None, F.from_numpy(np.zeros(box, S)), ([s.start for s in w], [s.stop for s in w]))
    q, b, minv, x = (F.from_numpy(np.full(box, v, S)) for v in (1.0, 2.0, 3.0, 4.0))
    out = nh.torch.full((2,), -7.0, dtype=nh.torch.float64, device="cuda")
    g = C.byref(level.geom)
    E = nh.capi.EINVAL
    call = lambda *a, pair=(nh.capi.F32, nh.capi.F64): nh.lib.neptune_hip_mg_smooth_dot_wide(pair[0], pair[1], g, *a, None)
    n_bytes = int(np.prod(box)) * 4
    good = (q.ptr, b.ptr, minv.ptr, x.ptr)
    for pair in ((nh.capi.F64, nh.capi.F64), (nh.capi.F32, nh.capi.F32), (nh.capi.F64, nh.capi.F32)):
        assert call(*good, out.data_ptr(), pair=pair) == E, pair
    assert call(*good, None) == E
    for f in (q, b, minv, x):
        assert call(*good, f.ptr) == E
        assert call(*good, f.ptr + n_bytes - 8) == E
    assert call(x.ptr, b.ptr, minv.ptr, x.ptr, out.data_ptr()) == E
    assert call(*good, out.data_ptr() + 4) == E
    level.minv = minv
    with pytest.raises(ValueError, match="float32"):
        nh.mg.smooth_dot_wide(level, q, b, F.from_numpy(np.zeros(box, D)))
    nh.torch.cuda.synchronize()
    assert float(out[0]) == -7.0 and bool((x.tensor == 4.0).all()) and bool((q.tensor == 1.0).all())


# ---------------------------------------------------------------- the narrowing of the set-up
def edge_values(with_nan: bool):
    """f64 values whose narrowing to f32 exercises every rule of the definition"""
    two = lambda e: math.ldexp(1.0, e)
    big = float(np.finfo(S).max)
    v = [1.0 + two(-24),                    # a tie between 1 and 1 + 2^-23: down, to the even mantissa
         1.0 + 3.0 * two(-24),              # a tie between 1 + 2^-23 and 1 + 2^-22: up, to the even mantissa
         -(1.0 + two(-24)), -(1.0 + 3.0 * two(-24)),
         1.0 + two(-24) + two(-52),         # just above the tie: up
         1.0 + 3.0 * two(-24) - two(-52),   # just below the tie: down
         1e-40, -1e-40,                     # f32's subnormal range
         two(-149),                         # the smallest subnormal, exact
         two(-150),                         # a tie between 0 and 2^-149: to 0
         -two(-150),                        # ... to -0
         3.0 * two(-150),                   # a tie between 2^-149 and 2^-148: to 2^-148
         two(-150) * (1.0 + two(-52)),      # just above half the smallest subnormal: to 2^-149
         two(-126) - two(-150),             # a tie between the largest subnormal and the smallest normal: to 2^-126
         1e-46, -1e-46,                     # below half the smallest subnormal: to +-0
         1e300, -1e300,                     # beyond f32's range: +-inf
         big + two(103),                    # f32's maximum plus half an ulp, a tie: to the even mantissa, which is +inf
         big + two(103) - two(75),          # just below it: f32's maximum
         -(big + two(103)),
         -0.0, 0.0]
    if with_nan:
        v.append(float("nan"))
    return v


def _setup_problem(nh, name):
    """-> (the restatement's Problem, the outer entry, the inner entries): two levels of the star operator"""
    spec = SETUPS[name]
    t64 = _text(*spec[0], D)
    t32 = [_text(*lv, S) for lv in spec]
    mg_device.prefetch([(t64, True)] + [(t, False) for t in t32])
    levels = []
    for l, (text, (box, lo, m)) in enumerate(zip(t32, spec)):
        w = _where(lo, m)
        levels.append(rst.Level(rst.Operator(text), box, w, mgc.minv_field(box, w, S, 0.8, outside=0.0 if l == 0 else np.nan), S))
    if len(spec[0][0]) == 2:
        levels[0].axes = (1,)
    entry64 = mg_device.entry(nh, t64, True)
    entries32 = [mg_device.entry(nh, t) for t in t32]
    return mx.Problem(rst.Operator(t64), levels), entry64, entries32


@pytest.mark.parametrize("with_nan", [True, False], ids=["nan", "inf"])
@pytest.mark.parametrize("name", sorted(SETUPS))
def test_the_set_up_narrows_as_the_definition_says(nh, name, with_nan):
    if name not in nh.setups:
        nh.setups[name] = _setup_problem(nh, name)
    P, entry64, entries32 = nh.setups[name]
    values = edge_values(with_nan)
    b = helpers.hash_field(P.shape, D, seed=17)          # b outside Omega is never read: it keeps its hashed values
    inside = b[P.where].copy().reshape(-1)
    assert inside.size >= 2 * len(values)
    inside[1:1 + 2 * len(values):2] = values             # every other cell of Omega from its second on
    b[P.where] = inside.reshape(b[P.where].shape)
    x0 = np.zeros(P.shape, D)
    x, r, r32, z32, rr0_ref = rst.store_residual(P, x0, b)
    # what the issue states of the restatement itself: from x = 0, r is b on Omega
    assert bits_equal(r[P.where], b[P.where]) and bits_equal(r32[P.where], rst.narrow(b[P.where]))     # narrow is .astype(float32)
    assert np.isinf(r32).sum() == 4 and (np.isnan(r32).sum() == 1) == with_nan
    subnormal = (r32 != 0) & (np.abs(r32) < np.finfo(S).tiny)
    assert subnormal.sum() >= 5 and ((z32 != 0) & (np.abs(z32) < np.finfo(S).tiny)).sum() >= 2
    dev = mx.device_problem(nh, P, entry64, entries32, x0, b)
    res = nh.mg.cg_solve_mixed(dev.outer, dev.h, dev.x, dev.b, max_iters=0, work=dev.work)
    nh.torch.cuda.synchronize()
    done, rr0, rr_last = res
    got_r, got_r32, got_z32 = dev.work[0].numpy(), dev.h.b[0].numpy(), dev.h.x[0].numpy()
    print(f"{name}: rr0 = {rr0!r} (restatement {rr0_ref[0]!r})")
    assert done == 0 and nh.mg.cg_counts() == (0, 0, 0, 0)
    assert (math.isnan(rr0) and math.isnan(rr_last)) if with_nan else (rr0 == math.inf and rr_last == math.inf)
    assert math.isnan(rr0_ref[0]) if with_nan else rr0_ref[0] == math.inf
    assert bits_equal(got_r, r), "r: " + mismatch_report(got_r, r)
    assert bits_equal(got_r32, r32), "r32: " + mismatch_report(got_r32, r32)
    assert bits_equal(got_z32, z32), "z32: " + mismatch_report(got_z32, z32)
    outside = np.ones(P.shape, bool)
    outside[P.where] = False
    for a in (got_r, got_r32, got_z32):
        assert bits_equal(a[outside], np.zeros(int(outside.sum()), a.dtype))
    assert bits_equal(dev.x.numpy(), x0) and bits_equal(dev.b.numpy(), b)
