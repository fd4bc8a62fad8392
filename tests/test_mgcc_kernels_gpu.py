"""The two transfer kernels on cell-centred level pairs (neptune_hip_mg_restrict / _prolong_add) against the
NumPy restatement of tests/mg_restatement.py: each kernel alone, bit for bit on every cell of every field, the untouched cells
outside Omega included.  On the parent commit every HALVED pair is NEPTUNE_HIP_EINVAL, so every test here fails there.

Shapes: the smallest at which the kernels can go wrong.  Rank 3: fine box 9 x 18 x 268, Omega 6 x 14 x 262 at (1, 2, 3) onto
3 x 7 x 131 under each of the 7 subsets of halved axes (the others kept) -- unequal rims, the fine row crosses the 256-cell
chunk with a 6-cell tail.  Rank 2: 14 x 524 onto 7 x 262, where the coarse row crosses the chunk.  Rank 1: 524 onto 262.  A
coarse grid one cell thick: 2 x 6 x 130 -> 1 x 3 x 65.  f64 and f32.

Alignment of the pair (2 j, 2 j + 1) that a lane of the restriction loads -- one load of 2 sizeof(T) where the row's first
Omega cell is aligned to that, two loads otherwise, the same bits either way.  All fields start 8 bytes into larger
allocations; with Omega's corner at 3 along the contiguous axis and an even pitch that makes the f32 pair misaligned and the
f64 pair aligned ((1 + 3) * 8 bytes), so the full mask runs once more at allocation offset 0 with the same corner (f64
misaligned), with an even corner at offset 0 (both aligned), and on a box of odd pitch 269, where the alignment alternates
from row to row.  test_the_cases_cover_both_load_paths computes this from the cases themselves.

The inputs hold -0 in places and NaN on every cell the definition says is not read, which is everything outside either
Omega: outside the fine Omega for the restriction, outside the coarse Omega for the prolongation, and the coarse b and x on
Omega before the restriction."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import dev, field
from mg_restatement import Halved

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
})
F64, F32 = np.float64, np.float32
RUNS = [(n, d, 8) for n in CASES if n != "even-corner" for d in (F64, F32)] + \
       [(n, d, 0) for n in ("r3-012", "even-corner", "odd-pitch") for d in (F64, F32)]
IDS = [f"{n}-{np.dtype(d).name}" + ("-offset" if o else "") for n, d, o in RUNS]


def test_the_cases_cover_both_load_paths():
    """per element type: some run whose every fine row starts a pair aligned to 2 sizeof(T), some run with none aligned, and
    one where the alignment alternates -- from the cases' own numbers (allocations are aligned to 16 bytes at least)"""
    seen = {F64: set(), F32: set()}
    for name, dtype, offset in RUNS:
        fbox, flo, fm, axes, _ = CASES[name]
        if len(fbox) - 1 not in axes:
            continue
        size = np.dtype(dtype).itemsize
        pitch = fbox[-1]
        rows = int(np.prod(fbox[:-1])) if len(fbox) > 1 else 1
        starts = {(offset + (r * pitch + flo[-1]) * size) % (2 * size) == 0 for r in range(min(rows, 4))}
        seen[dtype].add("mixed" if len(starts) == 2 else "aligned" if True in starts else "misaligned")
    assert seen[F64] == seen[F32] == {"aligned", "misaligned", "mixed"}, seen


@pytest.fixture(scope="module")
def nh(built_libs):
    return mg_device.namespace()


def Geometry(nh, name, dtype):
    fbox, flo, fm, axes, clo = CASES[name]
    cm = tuple(m // 2 if d in axes else m for d, m in enumerate(fm))
    return mg_device.Geometry(nh, (fbox, flo, fm), (mg_device.unequal_rims(clo, cm), clo, cm), dtype, axes)


@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS)
def test_restrict(nh, name, dtype, offset):
    G = Geometry(nh, name, dtype)
    assert nh.mg.coarsened_axes(G.fine, G.coarse) == G.axes == nh.mg.halved_axes(G.fine, G.coarse)
    b_f = field(G.fine_shape, dtype, 21, G.fw, np.nan)       # nothing outside the fine Omega is read
    q_f = field(G.fine_shape, dtype, 22, G.fw, np.nan)
    b_c = field(G.coarse_shape, dtype, 23, G.cw, inside=np.nan)      # what the coarse Omega held does not matter
    x_c = field(G.coarse_shape, dtype, 24, G.cw, inside=np.nan)
    for a in (b_c, x_c):
        a[tuple(0 for _ in a.shape)] = np.nan
    want_b, want_x = rst.restrict(b_f, q_f, G.fw, 4.0, b_c, x_c, G.cw, Halved(G.axes))
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
    x_c = field(G.coarse_shape, dtype, 31, G.cw, np.nan)     # no coarse cell outside the coarse Omega is read
    x_f = field(G.fine_shape, dtype, 32)
    x_f[tuple(0 for _ in x_f.shape)] = np.nan
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw, Halved(G.axes))
    xd = dev(nh, x_f, offset)
    nh.mg.prolong_add(G.fine, G.coarse, dev(nh, x_c, offset), xd)
    nh.torch.cuda.synchronize()
    got = xd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    assert np.isfinite(got[G.fw]).all()


@pytest.mark.parametrize("dtype", [F64, F32])
def test_minus_zero_and_nan_go_through(nh, dtype):
    """d = -0 on a pair of fine columns comes out as -0 on its coarse column (-0 + -0 = -0, 0.5 * -0 = -0, rscale * -0 = -0), a
    NaN in one fine cell reaches its one coarse cell only; the prolongation hands the coarse -0 / NaN to exactly the fine
    cells the coarse cell covers"""
    G = Geometry(nh, "r3-012", dtype)
    G.fine.rscale = 1.0
    b_f = np.ones(G.fine_shape, dtype)
    q_f = np.zeros(G.fine_shape, dtype)
    k0 = G.fw[2].start
    b_f[:, :, k0 + 10:k0 + 12] = -0.0                         # the fine columns 10, 11 -> the coarse column 5
    b_f[G.fw[0].start + 2, G.fw[1].start + 4, k0 + 261] = np.nan      # fine (2, 4, 261) -> coarse (1, 2, 130)
    zeros, ones = np.zeros(G.coarse_shape, dtype), np.ones(G.coarse_shape, dtype)
    want_b, _ = rst.restrict(b_f, q_f, G.fw, 1.0, zeros, ones, G.cw, Halved(G.axes))
    bd, xd = dev(nh, zeros, 0), dev(nh, ones, 0)
    nh.mg.restrict(G.fine, G.coarse, dev(nh, b_f, 0), dev(nh, q_f, 0), bd, xd)
    nh.torch.cuda.synchronize()
    got = bd.numpy()
    assert bits_equal(got, want_b), mismatch_report(got, want_b)
    inner = got[G.cw]
    assert np.signbit(inner[:, :, 5]).all() and (inner[:, :, 5] == 0).all()
    assert np.isnan(inner).sum() == 1 and np.isnan(inner[1, 2, 130])
    assert (np.delete(inner, [5, 130], axis=2) == 1).all()
    x_f = np.full(G.fine_shape, -0.0, dtype)
    want = rst.prolong_add(got, G.cw, x_f, G.fw, Halved(G.axes))
    fd = dev(nh, x_f, 0)
    nh.mg.prolong_add(G.fine, G.coarse, bd, fd)
    nh.torch.cuda.synchronize()
    out = fd.numpy()
    assert bits_equal(out, want), mismatch_report(out, want)
    fine = out[G.fw]
    assert np.signbit(fine[:, :, 10:12]).all() and (fine[:, :, 10:12] == 0).all()       # -0 + -0 = -0
    assert np.isnan(fine).sum() == 8 and np.isnan(fine[2:4, 4:6, 260:262]).all()


def test_refusals_on_device_pointers(nh):
    G = Geometry(nh, "r3-012", np.float64)
    F = nh.fields.DeviceField
    bf, qf, xf = (F.from_numpy(np.full(G.fine_shape, 3.0)) for _ in range(3))
    bc, xc = (F.from_numpy(np.full((5, 9, 134), 5.0)) for _ in range(2))
    lib, E, f64 = nh.lib, nh.capi.EINVAL, nh.capi.F64
    like_f, like_c = F.from_numpy(np.zeros(G.fine_shape)), F.from_numpy(np.zeros((5, 9, 134)))
    # the mixed pair: fine Omega 6 x 15 x 262 onto 3 x 7 x 131 -- dimensions 0 and 2 halved, dimension 1 coarsened
    mixed = nh.mg.Level(None, like_f, ([1, 2, 3], [7, 17, 265])).geom
    gc = nh.mg.Level(None, like_c, ([1, 1, 2], [4, 8, 133])).geom
    gf = G.fine.geom
    pairs = [(mixed, gc),
             (gf, gf),                                                           # all kept
             (gf, nh.mg.Level(None, like_c, ([1, 1, 2], [4, 8, 132])).geom)]     # dimension 2 in no state: 262 onto 130
    for g_fine, g_coarse in pairs:
        assert lib.neptune_hip_mg_restrict(f64, C.byref(g_fine), C.byref(g_coarse), bf.ptr, qf.ptr, 4.0, bc.ptr, xc.ptr, None) == E
        assert lib.neptune_hip_mg_prolong_add(f64, C.byref(g_fine), C.byref(g_coarse), xc.ptr, xf.ptr, None) == E
        for query in (lib.neptune_hip_mg_coarsened_axes, lib.neptune_hip_mg_halved_axes):
            mask = C.c_int(-7)
            assert query(C.byref(g_fine), C.byref(g_coarse), C.byref(mask)) == E and mask.value == -7
    # the good pair is refused for its other faults
    assert lib.neptune_hip_mg_restrict(f64, C.byref(gf), C.byref(gc), bf.ptr, qf.ptr, 4.0, bc.ptr, bc.ptr, None) == E
    assert lib.neptune_hip_mg_restrict(f64, C.byref(gf), C.byref(gc), bf.ptr, qf.ptr, float("inf"), bc.ptr, xc.ptr, None) == E
    assert lib.neptune_hip_mg_prolong_add(f64, C.byref(gf), C.byref(gc), xf.ptr, xf.ptr, None) == E
    assert lib.neptune_hip_mg_prolong_add(f64, C.byref(gc), C.byref(gf), xc.ptr, xf.ptr, None) == E       # the wrong way round
    nh.torch.cuda.synchronize()
    for f, v in ((bf, 3.0), (qf, 3.0), (xf, 3.0), (bc, 5.0), (xc, 5.0)):
        assert bool((f.tensor == v).all())
    # ... and accepted as it stands
    mask = C.c_int(-7)
    assert lib.neptune_hip_mg_halved_axes(C.byref(gf), C.byref(gc), C.byref(mask)) == nh.capi.OK and mask.value == 0b111
