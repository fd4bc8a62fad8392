"""The linear prolongation kernel of a cell-centred pair alone (neptune_hip_mg_prolong_add_linear) against the
NumPy restatement of tests/mg_restatement.py: bit for bit on every cell of the fine field, the untouched cells outside Omega
included.  On the parent commit the library lacks the export, so every test here fails there.

Shapes: those of test_mgcc_kernels_gpu.py -- rank 3, fine box 9 x 18 x 268, Omega 6 x 14 x 262 at (1, 2, 3) onto 3 x 7 x 131 under
each of the 7 subsets of halved axes (the fine row crosses the 256-cell chunk with a 6-cell tail); an even corner; a box of
odd pitch 269; rank 2, 14 x 524 onto 7 x 262; rank 1; `thin`, whose coarse Omega is 1 x 3 x 65, so both neighbours along
dimension 0 are ghosts -- and `long`, rank 3 with Omega 2 x 4 x 524 -> 1 x 2 x 262: the COARSE row crosses the 256-cell chunk of
the pair form, with a 6-cell tail.  f64 and f32.

Every case runs under a pattern of rules and under its complement, so every face meets EVEN and ODD.  The kernel has two
forms along the contiguous axis -- halved, the lane owns a pair of fine cells (x_f accessed as one 2 sizeof(T) access where
the row's first Omega cell is aligned to that, as two otherwise); kept, one cell per lane -- and
test_the_cases_reach_every_form computes from the cases themselves that both are run, the pair form with rows all aligned,
none aligned and alternating, per element type (allocation offsets 0 and 8 bytes).

The inputs hold -0 in places, NaN on every coarse cell outside the coarse Omega and on every fine cell outside the fine
Omega, and finite values inside."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mg_device
import mg_restatement as rst
from helpers import bits_equal, mismatch_report
from mg_device import dev
from mg_restatement import EVEN, Halved, Linear, ODD

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
})
F64, F32 = np.float64, np.float32
PATTERN = ((EVEN, ODD), (ODD, EVEN), (EVEN, EVEN))     # per dimension (low, high), the last `rank` entries read from the right
RUNS = [(n, d, 8) for n in CASES if n != "even-corner" for d in (F64, F32)] + \
       [(n, d, 0) for n in ("r3-012", "even-corner", "odd-pitch") for d in (F64, F32)]
IDS = lambda runs: [f"{n}-{np.dtype(d).name}" + ("-offset" if o else "") for n, d, o in runs]


def _rim(name, complemented):
    rank = len(CASES[name][0])
    rim = (PATTERN * 2)[3 - rank + (1 if name == "thin" else 0):][:rank]       # `thin` shifted: another face meets ODD first
    return rst.complement(rim) if complemented else tuple(rim)


def test_the_cases_reach_every_form():
    """from the cases' own numbers (allocations are aligned to 16 bytes at least): the kept form and, per element type, the
    pair form with every fine row's first Omega cell aligned to 2 sizeof(T), with none, and alternating; a coarse row beyond
    one chunk of the pair form; a coarse Omega one cell thick"""
    last_halved = lambda n: len(CASES[n][0]) - 1 in CASES[n][3]
    assert {d for n, d, _ in RUNS if not last_halved(n)} == {F64, F32}
    seen = {F64: set(), F32: set()}
    for name, dtype, offset in RUNS:
        fbox, flo, fm, axes, _ = CASES[name]
        if not last_halved(name):
            continue
        size = np.dtype(dtype).itemsize
        rows = int(np.prod(fbox[:-1])) if len(fbox) > 1 else 1
        starts = {(offset + (r * fbox[-1] + flo[-1]) * size) % (2 * size) == 0 for r in range(min(rows, 4))}
        seen[dtype].add("mixed" if len(starts) == 2 else "aligned" if True in starts else "misaligned")
    assert seen[F64] == seen[F32] == {"aligned", "misaligned", "mixed"}, seen
    assert any(last_halved(n) and CASES[n][2][-1] // 2 > 256 and len(CASES[n][0]) == 3 for n in CASES)
    assert any(m // 2 == 1 for n in CASES for d, m in enumerate(CASES[n][2]) if d in CASES[n][3])
    # every face meets both rules: a pattern and its complement
    for name in CASES:
        assert all({a, b} == {EVEN, ODD} for p, q in zip(_rim(name, False), _rim(name, True)) for a, b in zip(p, q))


@pytest.fixture(scope="module")
def nh(built_libs):
    return mg_device.namespace()


def Geometry(nh, name, dtype, rim=None):
    fbox, flo, fm, axes, clo = CASES[name]
    cm = tuple(m // 2 if d in axes else m for d, m in enumerate(fm))
    setting = {} if rim is None else dict(prolong="linear", faces=rst.faces_of(rim))
    return mg_device.Geometry(nh, (fbox, flo, fm), (mg_device.unequal_rims(clo, cm), clo, cm), dtype, axes, **setting)


def field(shape, dtype, seed, where):
    """hashed values with -0 sprinkled in on `where`, NaN on every other cell"""
    return mg_device.field(shape, dtype, seed, where, np.nan)


def _run(nh, name, dtype, offset, complemented):
    rim = _rim(name, complemented)
    G = Geometry(nh, name, dtype, rim)
    assert nh.mg.halved_axes(G.fine, G.coarse) == G.axes
    x_c = field(G.coarse_shape, dtype, 31, G.cw)             # no coarse cell outside the coarse Omega is read
    x_f = field(G.fine_shape, dtype, 32, G.fw)               # no fine cell outside the fine Omega is written
    assert np.isfinite(x_c[G.cw]).all() and np.signbit(x_c[G.cw][x_c[G.cw] == 0]).any()
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw, Linear(G.axes, rim))
    xd = dev(nh, x_f, offset)
    nh.mg.prolong_add(G.fine, G.coarse, dev(nh, x_c, offset), xd)
    nh.torch.cuda.synchronize()
    got = xd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    assert np.isfinite(got[G.fw]).all()
    return got


@pytest.mark.parametrize("complemented", [False, True], ids=["rules", "complement"])
@pytest.mark.parametrize("name,dtype,offset", RUNS, ids=IDS(RUNS))
def test_prolong_add_linear(nh, name, dtype, offset, complemented):
    _run(nh, name, dtype, offset, complemented)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_minus_zero_and_the_exact_sign_flip(nh, dtype):
    """x_c = -0 everywhere: an interior fine cell gets -0 (0.75 * -0 + 0.25 * -0), a cell on an ODD face +0 (its ghost is
    -(-0) = +0 and -0 + +0 = +0), on an EVEN face -0; with x_f = -0 the sum keeps those signs.  One NaN-free coarse spike of
    8 next to an ODD low corner comes out as 8 * (1/2)^3 in the corner cell -- the ghosts of the later dimensions are the
    intermediates' own"""
    rim = ((ODD, EVEN), (ODD, EVEN), (ODD, EVEN))
    G = Geometry(nh, "r3-012", dtype, rim)
    x_c = np.full(G.coarse_shape, np.nan, dtype)
    x_c[G.cw] = -0.0
    x_f = np.full(G.fine_shape, -0.0, dtype)
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw, Linear(G.axes, rim))
    fd = dev(nh, x_f, 0)
    nh.mg.prolong_add(G.fine, G.coarse, dev(nh, x_c, 0), fd)
    nh.torch.cuda.synchronize()
    got = fd.numpy()
    assert bits_equal(got, want), mismatch_report(got, want)
    inner = got[G.fw]
    assert (inner == 0).all()
    on_odd_face = np.zeros(inner.shape, bool)
    on_odd_face[0], on_odd_face[:, 0], on_odd_face[:, :, 0] = True, True, True
    assert not np.signbit(inner[on_odd_face]).any() and np.signbit(inner[~on_odd_face]).all()
    x_c[G.cw] = 0.0
    x_c[G.cw[0].start, G.cw[1].start, G.cw[2].start] = 8.0
    fd = dev(nh, np.zeros(G.fine_shape, dtype), 0)
    nh.mg.prolong_add(G.fine, G.coarse, dev(nh, x_c, 0), fd)
    nh.torch.cuda.synchronize()
    inner = fd.numpy()[G.fw]
    assert inner[0, 0, 0] == 1.0 and inner[1, 1, 1] == 8.0 * 0.75 ** 3 and inner[2, 2, 2] == 8.0 * 0.25 ** 3
    assert inner[0, 1, 2] == 8.0 * 0.5 * 0.75 * 0.25 and (inner[4:] == 0).all() and (inner[:, 4:] == 0).all() and (inner[:, :, 4:] == 0).all()


def test_kind_constant_and_unread_rules(nh):
    """through neptune_hip_mg_prolong_add_linear: kind CONSTANT is neptune_hip_mg_prolong_add whatever the rules hold; on a
    rank-2 pair the rules of dimension 2 are not read"""
    lib, f64 = nh.lib, nh.capi.F64
    G = Geometry(nh, "r2", F64)
    x_c, x_f = field(G.coarse_shape, F64, 41, G.cw), field(G.fine_shape, F64, 42, G.fw)
    p = nh.capi.MgProlong()
    p.kind = nh.capi.MG_PROLONG_CONSTANT
    for d in range(3):
        p.rim_lo[d], p.rim_hi[d] = 9, -9
    xd = dev(nh, x_f, 0)
    assert lib.neptune_hip_mg_prolong_add_linear(f64, C.byref(G.fine.geom), C.byref(G.coarse.geom), C.byref(p), dev(nh, x_c, 0).ptr, xd.ptr,
                                                 None) == nh.capi.OK
    nh.torch.cuda.synchronize()
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw, Halved(G.axes))
    assert bits_equal(xd.numpy(), want), mismatch_report(xd.numpy(), want)
    p.kind = nh.capi.MG_PROLONG_LINEAR
    p.rim_lo[0], p.rim_hi[0], p.rim_lo[1], p.rim_hi[1] = ODD, EVEN, EVEN, ODD
    xd = dev(nh, x_f, 0)
    assert lib.neptune_hip_mg_prolong_add_linear(f64, C.byref(G.fine.geom), C.byref(G.coarse.geom), C.byref(p), dev(nh, x_c, 0).ptr, xd.ptr,
                                                 None) == nh.capi.OK
    nh.torch.cuda.synchronize()
    want = rst.prolong_add(x_c, G.cw, x_f, G.fw, Linear(G.axes, ((ODD, EVEN), (EVEN, ODD))))
    assert bits_equal(xd.numpy(), want), mismatch_report(xd.numpy(), want)


def test_refusals_on_device_pointers(nh):
    G = Geometry(nh, "r3-012", np.float64)
    F = nh.fields.DeviceField
    xf, xc = F.from_numpy(np.full(G.fine_shape, 3.0)), F.from_numpy(np.full(G.coarse_shape, 5.0))
    lib, E, f64, lin = nh.lib, nh.capi.EINVAL, nh.capi.F64, nh.capi.MG_PROLONG_LINEAR
    gf, gc = G.fine.geom, G.coarse.geom

    def prolong(kind, lo=(0, 0, 0), hi=(0, 0, 0)):
        p = nh.capi.MgProlong()
        p.kind = kind
        for d in range(3):
            p.rim_lo[d], p.rim_hi[d] = lo[d], hi[d]
        return p
    call = lambda p, g_fine=gf, g_coarse=gc, coarse=xc: lib.neptune_hip_mg_prolong_add_linear(
        f64, C.byref(g_fine), C.byref(g_coarse), C.byref(p) if p is not None else None, coarse.ptr, xf.ptr, None)
    assert call(None) == E and call(prolong(2)) == E and call(prolong(-1)) == E
    for d in range(3):
        lo, hi = [0, 0, 0], [1, 1, 1]
        lo[d] = 2
        assert call(prolong(lin, lo, hi)) == E
        lo[d], hi[d] = 0, -1
        assert call(prolong(lin, lo, hi)) == E
    # LINEAR on a vertex-centred pair: fine Omega 7 x 15 x 263 onto 3 x 7 x 131
    like_f = F.from_numpy(np.zeros(G.fine_shape))
    vertex = nh.mg.Level(None, like_f, ([1, 2, 3], [8, 17, 266])).geom
    assert call(prolong(lin), g_fine=vertex) == E
    assert call(prolong(lin), g_fine=gc, g_coarse=gf) == E                             # the wrong way round
    assert call(prolong(lin), coarse=xf) == E                                          # x_fine overlaps x_coarse
    nh.torch.cuda.synchronize()
    assert bool((xf.tensor == 3.0).all()) and bool((xc.tensor == 5.0).all())
    with pytest.raises(nh.capi.NeptuneHipError):
        bad = Geometry(nh, "r3-012", np.float64, ((EVEN, EVEN),) * 3)
        bad.fine.geom = vertex
        nh.mg.prolong_add(bad.fine, bad.coarse, xc, xf)
    # ... and accepted as it stands
    assert call(prolong(lin, (1, 0, 1), (0, 1, 0))) == nh.capi.OK
    nh.torch.cuda.synchronize()
    assert bool((xf.tensor[G.fw] != 3.0).any())
